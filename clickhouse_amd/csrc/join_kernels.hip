// join_kernels.hip — hash join build and probe on the device for one numeric key (HashJoin key64 family).
//
// Reference loops replaced (file:line in the reference checkout):
//   k_join_insert / k_join_fill   HashJoin::addBlockToJoin -> insertFromBlockImplTypeCase, Inserter::insertOne/insertAll,
//                                 RowRefList::insert            src/Interpreters/HashJoin/HashJoin.cpp:556-768,
//                                                               HashJoinMethodsImpl.h:220-281, HashJoinMethods.h:16-62, RowRefs.h:16-141
//   k_join_probe_* / k_join_emit  HashJoin::joinBlock -> joinRightColumns (findKey, addFoundRowAll, addNotFoundRow,
//                                 offsets_to_replicate, filter, max_joined_block_rows)
//                                                               HashJoin.cpp:1036-1101, HashJoinMethodsImpl.h:402-549,
//                                                               KnownRowsHolder.h:88-153, JoinFeatures.h:9-40
//
// Design (not a translation): RowRef{block*,row} becomes a 64-bit global row id (block_index << 32 | row); the
// RowRefList's arena-allocated 7-slot batches become one CSR array (per-key count -> exclusive scan -> fill); the
// serial "first row owns the cell" rule becomes atomicMin (atomicMax for any_take_last_row) on the cell's row id; the
// INNER ANY "each right row joins its first left row only" flag (setUsedOnce) becomes atomicMin of a running left-row
// sequence number.  The table is built once in chgpu_join_finish_build (IJoin::onBuildPhaseFinish), sized from the
// number of build rows, so no kernel ever has to grow it.
#include "chgpu_internal.h"
#include "radix_partition.h"

#include <cstdlib>

#include <algorithm>
#include <vector>

static constexpr u32 JT = 256;
static constexpr u64 NO_ROW = ~0ull;
static constexpr u32 NO_SLOT = ~0u;
// packed probe value of a cell with several rows: bit 63 | min(count, SAT) << 40 | CSR start (40 bits)
static constexpr u64 JV_MULTI = 1ull << 63;
static constexpr u64 JV_CNT_SAT = (1ull << 23) - 1;
static constexpr u64 JV_START_MASK = (1ull << 40) - 1;
typedef u64 jv2 __attribute__((ext_vector_type(2))); // a {key, value} cell: one 16-byte access

struct JoinCtrl
{
    unsigned long long n_keys;
    u32 has_zero;
    u32 pad;
    u64 consumed; // probe: left rows consumed
    u64 n_out;    // probe: appended rows
    unsigned long long max_key; // largest non-zero build key (picks the prefilter's mode)
};

struct JoinTable
{
    u64 * kv;        // [cap+1][2] interleaved {key (0 = empty; cell cap = the zero key), value}: a probe's random access
                     // fetches the key and the answer from ONE 16-byte cell (separate arrays cost two HBM transactions)
    u64 * first_row; // [cap+1] global row id of the first (ANY: min or max) inserted row
    u32 * cnt;       // [cap+1] rows per key (ALL)
    u64 * start;     // [cap+1] CSR start (ALL)
    u64 * used_by;   // [cap+1] left-row sequence that consumed this cell (INNER ANY)
    u64 * rowids;    // [inserted] CSR payload (ALL)
                     // value = the row id itself (unique key / ANY), or MULTI | count | CSR start
    u64 capacity;
    JoinCtrl * ctrl;
    // Probe prefilter: a bitmap of pf_mask+1 bits (16 per build row, 64 Ki..32 Mi bits) small enough to live in L2, tested
    // before the hash table, which does not fit L2 for any but tiny build sides.  Dense keys (max key <= pf_mask: dimension
    // surrogate keys) index it directly -- exact; otherwise one multiplicative hash -- a k=1 Bloom filter (~6 % false
    // positives).  It never produces a false negative, so results are unchanged; misses stop at an L2 hit.
    u32 * pf;
    u64 pf_mask;
};

struct PfView
{
    const u32 * words;
    u64 mask;
    bool dense;
};
__device__ __forceinline__ PfView jt_pf_view(const JoinTable & t)
{
    PfView v;
    v.words = t.pf;
    v.mask = t.pf_mask;
    v.dense = t.ctrl->max_key <= t.pf_mask;
    return v;
}
__device__ __forceinline__ u64 jt_pf_pos(const PfView & v, u64 key) { return v.dense ? key : ((key * 0x9E3779B97F4A7C15ull) >> 32) & v.mask; }
// false = certainly absent.  key != 0 (the zero key lives out of line and is answered by has_zero).
__device__ __forceinline__ bool jt_pf_maybe(const PfView & v, u64 key)
{
    // (build sides beyond 2 Mi rows get no prefilter: it would need more than L2 can hold -- C4's 1e7 keys with a 4 MB,
    //  27 %-false-positive filter probed 18 % slower than without)
    if (v.dense && key > v.mask)
        return false;
    const u64 pos = jt_pf_pos(v, key);
    return (v.words[pos >> 5] >> (pos & 31)) & 1;
}

// cell s holds a key (cell `capacity` is the zero key's, answered by has_zero)
__device__ __forceinline__ bool jt_occupied(const JoinTable & t, u64 s) { return s == t.capacity ? (t.ctrl->has_zero != 0) : (t.kv[2 * s] != 0); }

// The packed probe value of a found cell: the row id itself (one row), or MULTI | count | CSR start.  A count that does not fit its 23 bits
// saturates and is read from t.cnt[slot] instead.
__device__ __forceinline__ u64 jv_pack(u32 count, u64 start) { return JV_MULTI | ((u64)(count < JV_CNT_SAT ? count : JV_CNT_SAT) << 40) | (start & JV_START_MASK); }
__device__ __forceinline__ bool jv_single(u64 v) { return !(v & JV_MULTI); }
__device__ __forceinline__ const u64 * jv_run(const JoinTable & t, u64 v) { return t.rowids + (v & JV_START_MASK); } // !jv_single(v)
// RowRefList::rows of the matched cell
__device__ __forceinline__ u32 jv_rows(const JoinTable & t, u64 v, u32 slot)
{
    if (jv_single(v))
        return 1;
    const u64 c = (v >> 40) & JV_CNT_SAT;
    return c < JV_CNT_SAT ? (u32)c : t.cnt[slot];
}
// fn(row id) for the first `rows` rows of the cell (a single row: that one)
template <typename Fn>
__device__ __forceinline__ void jv_for_each_row(const JoinTable & t, u64 v, u32 rows, Fn && fn)
{
    if (jv_single(v))
    {
        fn(v);
        return;
    }
    const u64 * run = jv_run(t, v);
    for (u32 k = 0; k < rows; ++k)
        fn(run[k]);
}

// row id (block << 32 | row) -> position in the payload columns glued over all blocks.  The block must exist: callers that can meet the
// default row of a miss check `rowid >> 32 < n_blocks` first.
__device__ __forceinline__ u64 join_flat_row(const u64 * block_base, u64 n_blocks, u64 rowid)
{
    return n_blocks == 1 ? (rowid & 0xFFFFFFFFull) : block_base[rowid >> 32] + (rowid & 0xFFFFFFFFull);
}

struct BuildBlock
{
    u64 * keys = nullptr; // zero-extended keys on device (context pool)
    u8 * valid = nullptr; // NULL = all rows valid
    size_t keys_class = 0, valid_class = 0;
    u64 rows = 0;
    u64 base = 0;         // running position of this block's first row in slot_of_row
};

struct chgpu_join
{
    chgpu_ctx * ctx = nullptr;
    int key_type = CHGPU_U64;
    int kind = CHGPU_JOIN_INNER, strictness = CHGPU_STRICT_ALL, any_take_last_row = 0;
    std::vector<BuildBlock> blocks;
    u64 total_rows = 0;
    bool finished = false;     // the hash table exists (join_build_table)
    bool build_closed = false; // onBuildPhaseFinish was called: no more right blocks; the table itself is built by the first consumer that needs it
    JoinTable t{};
    void * table_mem = nullptr;
    size_t table_class = 0;
    u64 n_keys = 0;
    u64 inserted = 0;
    bool unique_keys = false; // no key has more than one build row (the CSR arrays are then untouched)
    u64 max_key = 0;          // largest non-zero build key / whether the zero key is present (read back once by finish_build)
    bool has_zero = false;
    u64 left_seq = 0; // running left-row sequence across joinBlock calls (INNER ANY)
    // RIGHT / FULL: JoinUsedFlags (src/Interpreters/HashJoin/JoinUsedFlags.h) -- one byte per build row in insertion order
    u8 * used = nullptr;
    size_t used_class = 0;
    u64 * block_base_dev = nullptr; // [n_blocks] first flat row of every build block
    size_t base_class = 0;
    // Key set only (join_build_keyset): the exact bitmap over [0, max_key] of a build side of <= 4-byte keys, built WITHOUT the hash table
    // for consumers that only ask "is the key present" (the SEMI / ANTI steps of chgpu_join_probe_chain).  Superseded by t.pf once the
    // table exists.
    u32 * ks_pf = nullptr;
    size_t ks_class = 0;
    u64 ks_bits = 0;
    bool ks_ready = false;
    // the same key set with the build ROW of every key beside it (dense surrogate keys, unique, one build block): dm_rows[key] = row or
    // 0xFFFFFFFF -- what a chain step that adds right columns needs instead of the hash table (join_chain.h, join_build_dense)
    u32 * dm_rows = nullptr;
    size_t dm_class = 0;
    bool dm_ready = false;
    unsigned long long * key_stats = nullptr; // device: {largest inserted key, zero key inserted}, kept up to date by k_join_stage_keys;
                                              // word [2]: the duplicate-key flag of a row-map build (k_join_dense_fill)
    size_t key_stats_class = 0;
    u64 stats_host[2] = {0, 0}; // the two words on the host, when a caller has fetched them for several joins at once (a chain)
    bool stats_known = false;
    bool dm_pending = false;    // the row map is filled but its duplicate flag has not been looked at yet
};

// the left-side behaviour of the four kinds: RIGHT probes like INNER, FULL like LEFT (JoinFeatures.h:20-40: add_missing for LEFT / FULL)
static inline int jf_left_kind(const chgpu_join * j) { return (j->kind == CHGPU_JOIN_LEFT || j->kind == CHGPU_JOIN_FULL) ? CHGPU_JOIN_LEFT : CHGPU_JOIN_INNER; }
static inline bool jf_track_used(const chgpu_join * j) { return j->kind == CHGPU_JOIN_RIGHT || j->kind == CHGPU_JOIN_FULL; }

// RIGHT ANY / RIGHT SEMI: the first left row to find a key takes ALL the right rows of that key, so the left row is replicated (JoinFeatures.h:28)
static inline bool jf_right_once(const chgpu_join * j) { return j->kind == CHGPU_JOIN_RIGHT && (j->strictness == CHGPU_STRICT_ANY || j->strictness == CHGPU_STRICT_SEMI); }
static inline bool jf_need_replication(const chgpu_join * j) { return j->strictness == CHGPU_STRICT_ALL || jf_right_once(j); } // JoinFeatures.h:28
static inline bool jf_need_filter(const chgpu_join * j)
{
    return !jf_need_replication(j)
        && (jf_left_kind(j) == CHGPU_JOIN_INNER || j->strictness == CHGPU_STRICT_SEMI || j->strictness == CHGPU_STRICT_ANTI); // JoinFeatures.h:32
}
static inline bool jf_add_missing(const chgpu_join * j) { return jf_left_kind(j) == CHGPU_JOIN_LEFT && j->strictness != CHGPU_STRICT_SEMI; } // :35

// What answers "is this key on the build side, and at which row": the finished table with its prefilter, or -- before any table is
// built -- the key set (join_build_keyset) and its row map (join_build_dense).
struct JoinKeySet
{
    const u32 * pf;        // prefilter words or NULL
    u64 pf_mask;
    bool dense;            // pf is an exact bitmap over [0, max_key]
    u64 dense_bits;        // max_key + 1 rounded up to whole words
    u64 max_key;
    bool has_zero;
    const u64 * kv;        // {key, value} cells of the hash table, or NULL
    u64 capacity;
    const u32 * dense_row; // or NULL: dense_row[key] = the build row of the key
};
static JoinKeySet join_key_set(const chgpu_join * j)
{
    JoinKeySet k{};
    k.pf = j->finished ? j->t.pf : j->ks_pf;
    k.pf_mask = j->finished ? j->t.pf_mask : j->ks_bits - 1;
    k.dense = j->finished ? (j->t.pf && j->max_key <= j->t.pf_mask) : j->ks_ready;
    k.dense_bits = (j->max_key + 32) / 32 * 32;
    k.max_key = j->max_key;
    k.has_zero = j->has_zero;
    k.kv = j->finished ? j->t.kv : nullptr;
    k.capacity = j->finished ? j->t.capacity : 0;
    k.dense_row = (!j->finished && j->dm_ready) ? j->dm_rows : nullptr;
    return k;
}
// The LDS bitmap filters (k_join_probe_filter_lds_multi, k_chain_lds) take dense 4-byte keys whose bitmap fits `max_slices` slices of
// `slice_bits` (the kernel's geometry), read with 16-byte key loads and 4-byte null-map loads, over enough rows to pay for the staging
static bool join_lds_filter_fits(const JoinKeySet & k, int key_type, u64 n, const void * keys, const void * null_map, u64 slice_bits, u32 max_slices)
{
    return k.dense && chgpu_type_size(key_type) == 4 && k.dense_bits <= max_slices * slice_bits && n >= (1u << 20) && (uintptr_t)keys % 16 == 0
        && (!null_map || (uintptr_t)null_map % 4 == 0);
}

// An output column under construction: freed on scope exit unless it was released to the caller
struct JoinOutCol
{
    chgpu_col * col = nullptr;
    JoinOutCol() = default;
    JoinOutCol(const JoinOutCol &) = delete;
    JoinOutCol & operator=(const JoinOutCol &) = delete;
    ~JoinOutCol() { chgpu_col_free(col); }
    chgpu_col * release()
    {
        chgpu_col * c = col;
        col = nullptr;
        return c;
    }
};

// ---------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 jload_key(const void * keys, int type, u64 i)
{
    switch (type)
    {
        case CHGPU_U32: case CHGPU_I32: return ((const u32 *)keys)[i];
        case CHGPU_U16: case CHGPU_I16: return ((const u16 *)keys)[i];
        case CHGPU_U8: case CHGPU_I8: return ((const u8 *)keys)[i];
        default: return ((const u64 *)keys)[i];
    }
}

// stats[0] = the largest inserted key, stats[1] = 1 when the zero key is inserted: what the key-set / row-map builds of join_chain.h size
// themselves by, gathered while the keys pass through anyway.  One atomic per WORKGROUP at most, and only when it would change the
// word (thousands of waves on two addresses cost more than the pass itself).  4-byte keys whose column and staging buffer are 16-byte
// aligned move four rows per lane (the dimension tables of a star join: 30 M customer keys at the rate of a copy).
__global__ __launch_bounds__(JT) void k_join_stage_keys(const void * __restrict__ keys, int type, const u8 * __restrict__ null_map,
                                                        const u8 * __restrict__ join_mask, u64 n, u64 * __restrict__ out_keys, u8 * __restrict__ out_valid,
                                                        unsigned long long * __restrict__ stats)
{
    u64 m = 0;
    u32 zero = 0;
    auto row = [&](u64 i, u64 k) {
        const bool valid = !(null_map && null_map[i]) && !(join_mask && !join_mask[i]); // HashJoinMethodsImpl.h:261-272
        if (out_valid)
            out_valid[i] = valid;
        if (valid)
        {
            m = k > m ? k : m;
            zero |= k == 0 ? 1u : 0u;
        }
    };
    const bool wide = (type == CHGPU_U32 || type == CHGPU_I32) && (((uintptr_t)keys | (uintptr_t)out_keys) & 15) == 0;
    if (wide)
    {
        typedef u32 v4d __attribute__((ext_vector_type(4)));
        typedef u64 v2q __attribute__((ext_vector_type(2)));
        const u64 quads = n / 4;
        for (u64 q = (u64)blockIdx.x * JT + threadIdx.x; q < quads; q += (u64)gridDim.x * JT)
        {
            const v4d k4 = __builtin_nontemporal_load((const v4d *)keys + q);
            __builtin_nontemporal_store(v2q{k4.x, k4.y}, (v2q *)out_keys + 2 * q);
            __builtin_nontemporal_store(v2q{k4.z, k4.w}, (v2q *)out_keys + 2 * q + 1);
            row(4 * q, k4.x), row(4 * q + 1, k4.y), row(4 * q + 2, k4.z), row(4 * q + 3, k4.w);
        }
        for (u64 i = quads * 4 + (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
        {
            const u64 k = ((const u32 *)keys)[i];
            out_keys[i] = k;
            row(i, k);
        }
    }
    else
        for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
        {
            const u64 k = jload_key(keys, type, i);
            out_keys[i] = k;
            row(i, k);
        }
    m = wave_reduce_max_u64(m);
    zero = __any(zero) ? 1u : 0u;
    __shared__ unsigned long long s_m;
    __shared__ u32 s_zero;
    if (threadIdx.x == 0)
        s_m = 0, s_zero = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
    {
        if (m)
            atomicMax(&s_m, (unsigned long long)m);
        if (zero)
            atomicOr(&s_zero, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        if (s_m > __hip_atomic_load(stats, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(stats, s_m);
        if (s_zero && !__hip_atomic_load(stats + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicOr(stats + 1, 1ull);
    }
}

// `claimed` tells the caller a new cell was taken; callers count claims in registers and add them to ctrl->n_keys once
// per wave when the kernel ends (a per-lane atomicAdd on that single address serialised the whole build: 6.3 ms for 1e7 rows).
__device__ __forceinline__ u32 jt_emplace(const JoinTable & t, u64 key, bool & claimed)
{
    claimed = false;
    if (key == 0)
    {
        if (t.ctrl->has_zero == 0 && atomicExch(&t.ctrl->has_zero, 1u) == 0)
            claimed = true;
        return (u32)t.capacity;
    }
    const u64 mask = t.capacity - 1;
    u64 slot = dev_intHash64(key) & mask;
    for (u64 step = 0; step < t.capacity; ++step)
    {
        u64 k = t.kv[2 * slot];
        if (k == 0)
        {
            k = atomicCAS((unsigned long long *)&t.kv[2 * slot], 0ull, (unsigned long long)key);
            if (k == 0)
            {
                claimed = true;
                return (u32)slot;
            }
        }
        if (k == key)
            return (u32)slot;
        slot = (slot + 1) & mask;
    }
    return NO_SLOT; // unreachable: capacity >= 2 * rows
}

// The open-addressing walk over [capacity] {key, value} cells for a NON-ZERO key: compare, stop at an empty cell, step.  It starts at
// `slot` with `step` cells already looked at by the caller (a staged look-up that has read the home cell itself) and returns the key's
// slot or NO_SLOT.  CELL: every step reads the whole 16-byte cell and a hit leaves the value word in `value` (the key and its answer in
// one transaction); otherwise only the 8-byte key word is read and `value` is left alone.
template <bool CELL>
__device__ __forceinline__ u32 jt_walk(const u64 * kv, u64 capacity, u64 key, u64 slot, u64 step, u64 & value)
{
    const u64 mask = capacity - 1;
    u32 at = NO_SLOT;
    for (; step < capacity; ++step)
    {
        u64 k;
        if constexpr (CELL)
        {
            const jv2 c = *(const jv2 *)(kv + 2 * slot);
            k = c.x;
            if (k == key)
                value = c.y;
        }
        else
            k = kv[2 * slot];
        if (k == key)
            at = (u32)slot;
        if (k == key || k == 0)
            break;
        slot = (slot + 1) & mask;
    }
    return at;
}

// -> the key's slot or NO_SLOT: the zero key's rule (it lives in cell `capacity`), the prefilter, the walk from the home slot
// PF: the table has a prefilter (kernels are instantiated both ways and the host picks: with the test compiled in but
// disabled at run time, the C4 probe -- whose 1e7-row build side has no prefilter -- ran 37 % slower)
template <bool PF, bool CELL>
__device__ __forceinline__ u32 jt_lookup(const JoinTable & t, const PfView & pf, u64 key, u64 & value)
{
    if (key == 0)
    {
        if (!t.ctrl->has_zero)
            return NO_SLOT;
        if constexpr (CELL)
            value = t.kv[2 * t.capacity + 1];
        return (u32)t.capacity;
    }
    if constexpr (PF)
        if (!jt_pf_maybe(pf, key))
            return NO_SLOT;
    return jt_walk<CELL>(t.kv, t.capacity, key, dev_intHash64(key) & (t.capacity - 1), 0, value);
}
template <bool PF>
__device__ __forceinline__ u32 jt_find(const JoinTable & t, const PfView & pf, u64 key)
{
    u64 unused;
    return jt_lookup<PF, false>(t, pf, key, unused);
}

// build pass 1: claim cells, count rows per key, record the owning row.
// The row that CLAIMS a cell (wins the compare-and-swap on its key) stores its row id with a plain store into the cell's value word --
// the same 16 bytes it has just touched -- and issues no further atomic.  Only later rows of the same key pay atomics (rows-per-key
// count, min / max row id).  A primary-key build side (every row claims) thus costs ONE device-scope atomic per row instead of
// three: the pass is bound by the ~2e10/s rate of scattered memory-side atomics, not by bandwidth.  ctrl->pad is set when any row found
// its key already present: without duplicates the CSR passes below (scan, fill, root-first) are skipped altogether.
__global__ __launch_bounds__(JT) void k_join_insert(JoinTable t, const u64 * __restrict__ keys, const u8 * __restrict__ valid, u64 n,
                                                    u64 block_index, int maps_all, int take_last, u32 * __restrict__ slot_of_row)
{
    u32 my_claims = 0; // nobody reads n_keys before the kernel ends: count in registers, one atomic per wave at the end
    u32 my_dups = 0;
    u64 my_max = 0;
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
    {
        u32 slot = NO_SLOT;
        bool claimed = false;
        if (!valid || valid[i])
        {
            my_max = keys[i] > my_max ? keys[i] : my_max;
            slot = jt_emplace(t, keys[i], claimed);
            if (slot != NO_SLOT)
            {
                const u64 rowid = (block_index << 32) | i;
                if (claimed)
                    t.kv[2 * (u64)slot + 1] = rowid; // nobody else writes this word before k_join_merge_claims / finalize read it
                else
                {
                    ++my_dups;
                    if (maps_all)
                    {
                        atomicAdd(&t.cnt[slot], 1u);                                              // RowRefList::rows beyond the claimer's
                        atomicMin((unsigned long long *)&t.first_row[slot], (unsigned long long)rowid); // the root RowRef = first inserted
                    }
                    else if (take_last)
                        atomicMax((unsigned long long *)&t.first_row[slot], (unsigned long long)(rowid + 1)); // stored +1 so 0 == unset
                    else
                        atomicMin((unsigned long long *)&t.first_row[slot], (unsigned long long)rowid);       // insertOne: first row wins
                }
            }
        }
        slot_of_row[i] = slot;
        my_claims += claimed;
    }
    // (a same-address atomic per wave and iteration costs ~10 ns each: 1.5 ms of a 1e7-row build)
    const u32 tot = wave_reduce_add_u32(my_claims), dups = wave_reduce_add_u32(my_dups);
    if ((threadIdx.x & 63) == 0 && tot)
        atomicAdd(&t.ctrl->n_keys, (unsigned long long)tot);
    if ((threadIdx.x & 63) == 0 && dups && t.ctrl->pad == 0)
        atomicOr(&t.ctrl->pad, 1u);
    my_max = wave_reduce_max_u64(my_max);
    if ((threadIdx.x & 63) == 0 && my_max)
        atomicMax(&t.ctrl->max_key, (unsigned long long)my_max);
}

// build pass 1b (only when some key has several rows): fold the claimers' row ids (value words) into first_row / cnt so the CSR passes
// see what three atomics per row used to leave there
__global__ __launch_bounds__(JT) void k_join_merge_claims(JoinTable t, int maps_all, int take_last)
{
    for (u64 s = (u64)blockIdx.x * JT + threadIdx.x; s <= t.capacity; s += (u64)gridDim.x * JT)
    {
        if (!jt_occupied(t, s))
            continue;
        const u64 claim = t.kv[2 * s + 1];
        if (maps_all)
        {
            t.cnt[s] += 1;
            t.first_row[s] = claim < t.first_row[s] ? claim : t.first_row[s];
        }
        else if (take_last)
            t.first_row[s] = claim + 1 > t.first_row[s] ? claim + 1 : t.first_row[s];
        else
            t.first_row[s] = claim < t.first_row[s] ? claim : t.first_row[s];
    }
}

// build pass 3: CSR fill
__global__ __launch_bounds__(JT) void k_join_fill(JoinTable t, const u32 * __restrict__ slot_of_row, u64 n, u64 block_index, u32 * __restrict__ cursor)
{
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
    {
        const u32 slot = slot_of_row[i];
        if (slot == NO_SLOT)
            continue;
        const u32 k = atomicAdd(&cursor[slot], 1u);
        t.rowids[t.start[slot] + k] = (block_index << 32) | i;
    }
}

// build pass 4: put the first-inserted row at the head of each key's run (RowRefList iteration starts at the root)
__global__ __launch_bounds__(JT) void k_join_root_first(JoinTable t)
{
    for (u64 s = (u64)blockIdx.x * JT + threadIdx.x; s <= t.capacity; s += (u64)gridDim.x * JT)
    {
        const u32 c = t.cnt[s];
        if (c < 2)
            continue;
        u64 * run = t.rowids + t.start[s];
        const u64 root = t.first_row[s];
        for (u32 k = 0; k < c; ++k)
            if (run[k] == root)
            {
                run[k] = run[0];
                run[0] = root;
                break;
            }
    }
}

// build pass 5: one 8-byte word per cell that answers a probe without touching cnt/start/rowids for unique keys.
// unique != 0: no key had a second row -- the value words already hold the claimers' row ids; only the prefilter is filled.
__global__ __launch_bounds__(JT) void k_join_finalize_values(JoinTable t, int maps_all, int take_last, int unique)
{
    const PfView pf = jt_pf_view(t); // every insert kernel has finished: max_key is final
    for (u64 s = (u64)blockIdx.x * JT + threadIdx.x; s <= t.capacity; s += (u64)gridDim.x * JT)
    {
        const bool occupied = jt_occupied(t, s);
        u64 v = NO_ROW;
        if (occupied && s != t.capacity && t.pf)
        {
            const u64 pos = jt_pf_pos(pf, t.kv[2 * s]);
            atomicOr(&t.pf[pos >> 5], 1u << (pos & 31));
        }
        if (unique)
        {
            if (!occupied)
                t.kv[2 * s + 1] = NO_ROW;
            continue;
        }
        if (occupied)
        {
            if (!maps_all)
                v = take_last ? t.first_row[s] - 1 : t.first_row[s];
            else
            {
                const u32 c = t.cnt[s];
                if (c == 1)
                    v = t.rowids[t.start[s]];
                else
                    v = jv_pack(c, t.start[s]);
            }
        }
        t.kv[2 * s + 1] = v;
    }
}

// prefilter bits straight from the build keys (after a slice build: unique keys, no NULLs, nothing else to finalise -- a pass over
// the build rows instead of k_join_finalize_values' pass over every cell)
__global__ __launch_bounds__(JT) void k_join_pf_fill(JoinTable t, const u64 * __restrict__ keys, u64 n)
{
    const PfView pf = jt_pf_view(t);
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
    {
        const u64 key = keys[i];
        if (key)
        {
            const u64 pos = jt_pf_pos(pf, key);
            atomicOr(&t.pf[pos >> 5], 1u << (pos & 31));
        }
    }
}

// largest staged build key (NULL rows staged as 0), for the dense-prefilter decision of build sides beyond 2 Mi rows
__global__ __launch_bounds__(JT) void k_join_max_key(const u64 * __restrict__ keys, u64 n, unsigned long long * __restrict__ out)
{
    u64 m = 0;
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
        m = keys[i] > m ? keys[i] : m;
    m = wave_reduce_max_u64(m);
    if ((threadIdx.x & 63) == 0 && m)
        atomicMax(out, (unsigned long long)m);
}

__global__ __launch_bounds__(JT) void k_fill_u64(u64 * p, u64 n, u64 v)
{
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
        p[i] = v;
}

enum { PV_ALL_INNER, PV_ALL_LEFT, PV_ANY_LEFT, PV_SEMI_LEFT, PV_ANTI_LEFT, PV_ANY_INNER, PV_ONCE_RIGHT, PV_ANTI_RIGHT };

// addNotFoundRow<add_missing>: a left row without a match is still a row of the result -- with a default right row (payload 0) for
// LEFT ALL / LEFT ANY, as the kept row of ANTI
__device__ __forceinline__ bool pv_miss_counts(int variant) { return variant == PV_ALL_LEFT || variant == PV_ANY_LEFT || variant == PV_ANTI_LEFT; }
// What one left key adds to a fused probe's count before its right rows are looked at: a miss counts itself where misses count; a hit
// of ANTI adds nothing.  -> true when the matched right rows are to be added (a row with a NULL key finds nothing,
// HashJoinMethodsImpl.h:451-452, but is still a left row of LEFT / ANTI joins: callers pass found = false for it)
__device__ __forceinline__ bool pv_account(int variant, bool found, u64 & cnt)
{
    if (!found)
    {
        cnt += pv_miss_counts(variant) ? 1 : 0;
        return false;
    }
    return variant != PV_ANTI_LEFT;
}

// a filter-only probe's kept rows -> ctrl->n_out: one atomic per wave that kept any
__device__ __forceinline__ void join_add_kept(JoinCtrl * ctrl, u32 kept)
{
    kept = wave_reduce_add_u32(kept);
    if ((threadIdx.x & 63) == 0 && kept)
        atomicAdd((unsigned long long *)&ctrl->n_out, (unsigned long long)kept);
}

// A JT-thread workgroup's {count, sum} in a fixed order: lane partials -> wave (shuffle tree) -> workgroup (LDS, wave order).  `sbits`
// carries the sum -- an integer, or the bits of a Float64 (FLOAT).  -> true in thread 0, whose cnt / sbits then hold the workgroup's.
template <bool FLOAT>
__device__ __forceinline__ bool join_fold_workgroup(u64 & cnt, u64 & sbits)
{
    __shared__ u64 sh_c[JT / 64], sh_s[JT / 64];
    cnt = wave_reduce_add_u64(cnt);
    if constexpr (FLOAT)
        sbits = (u64)__double_as_longlong(wave_reduce_add_f64(__longlong_as_double((long long)sbits)));
    else
        sbits = wave_reduce_add_u64(sbits);
    if ((threadIdx.x & 63) == 0)
    {
        sh_c[threadIdx.x >> 6] = cnt;
        sh_s[threadIdx.x >> 6] = sbits;
    }
    __syncthreads();
    if (threadIdx.x != 0)
        return false;
    u64 c = 0, si = 0;
    double sf = 0.0;
    for (u32 w = 0; w < JT / 64; ++w)
    {
        c += sh_c[w];
        if constexpr (FLOAT)
            sf += __longlong_as_double((long long)sh_s[w]);
        else
            si += sh_s[w];
    }
    cnt = c;
    sbits = FLOAT ? (u64)__double_as_longlong(sf) : si;
    return true;
}

// probe pass 0 (INNER ANY only): every matching left row bids for its right cell with its sequence number
template <bool PF>
__global__ __launch_bounds__(JT) void k_join_probe_bid(JoinTable t, const void * __restrict__ keys, int key_type, const u8 * __restrict__ null_map,
                                                       u64 n, u64 seq_base, u32 * __restrict__ slot_of_left)
{
    PfView pf{};
    if constexpr (PF)
        pf = jt_pf_view(t);
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
    {
        u32 slot = NO_SLOT;
        if (!(null_map && null_map[i]))
            slot = jt_find<PF>(t, pf, jload_key(keys, key_type, i));
        if (slot != NO_SLOT)
            atomicMin((unsigned long long *)&t.used_by[slot], (unsigned long long)(seq_base + i));
        slot_of_left[i] = slot;
    }
}

// probe pass 1: per left row, how many right rows get appended (and the filter byte).  A hit costs one random read (the 16-byte cell holds
// the key and its packed value word); the value is kept per left row so the emit pass streams instead of re-probing.
// Four rows per lane, stage by stage, every load of a stage unconditional (a row that is not looked up reads word / cell 0): a lane has four
// key loads, then four prefilter words, then four home cells in flight.  One row per lane and a probe loop per row left the kernel
// parked on s_waitcnt (2.55 ms for 1e8 probes of a 1e6-key table that needs 0.5 ms of traffic); only a row whose home cell holds
// another key walks on, by itself.
template <bool PF>
__global__ __launch_bounds__(JT) void k_join_probe_count(JoinTable t, int variant, const void * __restrict__ keys, int key_type,
                                                         const u8 * __restrict__ null_map, u64 n, u64 seq_base, int slots_known,
                                                         u32 * __restrict__ slot_of_left, u64 * __restrict__ val_of_left,
                                                         u32 * __restrict__ counts, u8 * __restrict__ filter)
{
    PfView pf{};
    if constexpr (PF)
        pf = jt_pf_view(t);
#ifndef JPC_R
#define JPC_R 4
#endif
    constexpr int R = JPC_R;
    const u64 stride = (u64)gridDim.x * JT;
    const u64 mask = t.capacity - 1;
    for (u64 i0 = (u64)blockIdx.x * JT + threadIdx.x; i0 < n; i0 += stride * R)
    {
        u64 key[R], val[R];
        u32 slot[R];
        bool in[R], look[R];
#pragma unroll
        for (int q = 0; q < R; ++q)
        {
            const u64 i = i0 + (u64)q * stride;
            in[q] = i < n;
            const u64 ic = in[q] ? i : n - 1;
            key[q] = 0;
            slot[q] = NO_SLOT;
            if (slots_known)
                slot[q] = slot_of_left[ic];
            else
                key[q] = jload_key(keys, key_type, ic);
            const bool is_null = null_map && null_map[ic]; // HashJoinMethodsImpl.h:451-452
            look[q] = in[q] && !slots_known && !is_null;
        }
        if (!slots_known)
        {
            bool zero[R];
            u64 home[R];
#pragma unroll
            for (int q = 0; q < R; ++q)
            {
                zero[q] = look[q] && key[q] == 0; // the zero key lives out of line (HashTable.h:874-898)
                look[q] = look[q] && key[q] != 0;
            }
            if constexpr (PF)
            {
                u32 pw[R];
                u64 pos[R];
#pragma unroll
                for (int q = 0; q < R; ++q)
                {
                    look[q] = look[q] && !(pf.dense && key[q] > pf.mask);
                    pos[q] = look[q] ? jt_pf_pos(pf, key[q]) : 0;
                    pw[q] = pf.words[pos[q] >> 5];
                }
#pragma unroll
                for (int q = 0; q < R; ++q)
                    look[q] = look[q] && ((pw[q] >> (pos[q] & 31)) & 1u);
            }
            jv2 c[R], c2[R];
#pragma unroll
            for (int q = 0; q < R; ++q)
            {
                home[q] = dev_intHash64(key[q]) & mask;
                c[q] = *(const jv2 *)(t.kv + 2 * (look[q] ? home[q] : 0));
                c2[q] = *(const jv2 *)(t.kv + 2 * (look[q] ? (home[q] + 1) & mask : 0)); // the next cell too: nearly always the same 64-byte sector
            }
#pragma unroll
            for (int q = 0; q < R; ++q)
            {
                val[q] = NO_ROW;
                if (look[q])
                {
                    if (c[q].x == key[q])
                    {
                        slot[q] = (u32)home[q];
                        val[q] = c[q].y;
                    }
                    else if (c[q].x == 0)
                        ;
                    else if (c2[q].x == key[q])
                    {
                        slot[q] = (u32)((home[q] + 1) & mask);
                        val[q] = c2[q].y;
                    }
                    else if (c2[q].x != 0)
                    {
                        // other keys in both cells: the rest of the walk (open-coded: through jt_walk this kernel needs 2 more VGPRs)
                        u64 sl = (home[q] + 2) & mask;
                        for (u64 step = 2; step < t.capacity; ++step)
                        {
                            const jv2 cc = *(const jv2 *)(t.kv + 2 * sl);
                            if (cc.x == key[q])
                            {
                                slot[q] = (u32)sl;
                                val[q] = cc.y;
                                break;
                            }
                            if (cc.x == 0)
                                break;
                            sl = (sl + 1) & mask;
                        }
                    }
                }
                else if (zero[q] && t.ctrl->has_zero)
                {
                    slot[q] = (u32)t.capacity;
                    val[q] = t.kv[2 * t.capacity + 1];
                }
            }
        }
        else
        {
#pragma unroll
            for (int q = 0; q < R; ++q)
            {
                const u64 v = t.kv[2 * (u64)(slot[q] != NO_SLOT ? slot[q] : 0) + 1];
                val[q] = slot[q] != NO_SLOT ? v : NO_ROW;
            }
        }
#pragma unroll
        for (int q = 0; q < R; ++q)
        {
            if (!in[q])
                continue;
            const u64 i = i0 + (u64)q * stride;
            const bool found = slot[q] != NO_SLOT;
            const u64 v = val[q];
            const u32 rows_here = found ? jv_rows(t, v, slot[q]) : 0;
            u32 c = 0;
            u8 f = 0;
            switch (variant)
            {
                case PV_ALL_INNER: c = rows_here; break;
                case PV_ALL_LEFT: c = found ? rows_here : 1; break;                   // addNotFoundRow<add_missing>: ++current_offset
                case PV_ANY_LEFT: c = 1; break;                                       // found row or default row
                case PV_SEMI_LEFT: c = found ? 1 : 0; f = found; break;
                case PV_ANTI_LEFT: c = found ? 0 : 1; f = !found; break;              // :515-519, :535-536
                case PV_ANY_INNER: c = (found && t.used_by[slot[q]] == seq_base + i) ? 1 : 0; f = (u8)c; break; // setUsedOnce, :498-510
                case PV_ONCE_RIGHT: c = (found && t.used_by[slot[q]] == seq_base + i) ? rows_here : 0; break;     // RIGHT ANY / SEMI: setUsedOnce + addFoundRowAll, :487-497
                case PV_ANTI_RIGHT: c = 0; f = 0; break;                              // RIGHT ANTI: found rows only set the flags (:515-519), nothing is emitted
            }
            counts[i] = c;
            val_of_left[i] = v;
            if (filter)
                filter[i] = f;
        }
    }
}

// LEFT SEMI / LEFT ANTI when the right side contributes no columns (the caller passed right_rowid == NULL; the reference's
// AddedColumns is empty then): only the filter byte and the number of kept rows are produced -- 1 byte written per left row
// instead of 21 (counts, packed values, offsets) plus a scan and an emit pass.  Four rows per lane are in flight.
template <bool PF>
__global__ __launch_bounds__(JT) void k_join_probe_filter(JoinTable t, int anti, const void * __restrict__ keys, int key_type,
                                                          const u8 * __restrict__ null_map, u64 n, u8 * __restrict__ filter, JoinCtrl * __restrict__ ctrl)
{
    PfView pf{};
    if constexpr (PF)
        pf = jt_pf_view(t);
#ifndef JPF_R
#define JPF_R 4
#endif
    constexpr int R = JPF_R;
    u32 kept = 0;
    const u64 stride = (u64)gridDim.x * JT;
    for (u64 i0 = (u64)blockIdx.x * JT + threadIdx.x; i0 < n; i0 += stride * R)
    {
        u64 key[R];
        bool in[R], ok[R];
#pragma unroll
        for (int q = 0; q < R; ++q)
        {
            const u64 i = i0 + (u64)q * stride;
            in[q] = i < n;
            ok[q] = in[q] && !(null_map && null_map[i]); // HashJoinMethodsImpl.h:451-452
            key[q] = in[q] ? jload_key(keys, key_type, i) : 0;
        }
#pragma unroll
        for (int q = 0; q < R; ++q)
        {
            if (!in[q])
                continue;
            bool found;
            if (PF && pf.dense && key[q] != 0)
                found = ok[q] && jt_pf_maybe(pf, key[q]); // a dense prefilter is exact: membership needs no table access
            else
                found = ok[q] && jt_find<PF>(t, pf, key[q]) != NO_SLOT;
            const u8 f = anti ? !found : found;             // :515-519, :535-536
            filter[i0 + (u64)q * stride] = f;
            kept += f;
        }
    }
    join_add_kept(ctrl, kept);
}

// The same filter-only probe for DENSE 4-byte keys (dimension surrogate keys: the prefilter bitmap IS the key set) with the bitmap
// staged in LDS, a slice of JPL_SLICE_BITS bits (150 KiB) of the key domain at a time.  From L2 the look-ups run at ~1.6e11/s
// chip-wide -- 64 lanes = 64 separate L2 requests -- i.e. 4.8 ms for the 750 M lineorder rows of SSB against the 0.6 ms the keys and
// filter bytes take to stream; LDS serves the same random bit reads an order of magnitude faster.
// A key set of one OR several slices is probed in ONE sweep over the rows.  One pass over all rows per slice would read the keys again
// from HBM each time and read back and rewrite the filter bytes of the passes before; here a workgroup takes a PART of 64 Ki rows through
// all slices before it moves on: the part's keys (16 bytes = four rows per lane and load, plain loads) come from HBM once and from L2 /
// Infinity Cache for the other slices, the hit bits of a thread's 64 rows wait in two registers between slices (a row's key lies in
// exactly one slice), and the null-map bytes are read and the filter bytes written once, with the last slice.  Between slices the
// workgroup reloads its 150 KiB of LDS from the bitmap (L2-resident); consecutive parts walk the slices in opposite directions, so the
// slice a part ends with is the one the next part starts with -- a single slice is staged once per workgroup.
static constexpr u32 JPL_SLICE_BITS = 150u * 1024u * 8u;
template <bool HAS_NULL>
__global__ __launch_bounds__(1024) void k_join_probe_filter_lds_multi(const u32 * __restrict__ pf_words, u32 dense_bits, u32 n_slices, int anti, int has_zero,
                                                                      const u32 * __restrict__ keys, const u8 * __restrict__ null_map, u64 n,
                                                                      u8 * __restrict__ filter, JoinCtrl * __restrict__ ctrl)
{
    extern __shared__ __attribute__((aligned(16))) u32 jpl_bits[];
    typedef u32 v4u __attribute__((ext_vector_type(4)));
    constexpr u32 JPM_QPT = 16;                // quads (of four rows) per thread and part: a thread's hit bits fill one 64-bit register
    constexpr u32 JPM_PART_Q = 1024 * JPM_QPT; // quads per part
    const u64 nq = n / 4; // whole groups of four rows; the last n % 4 rows are done at the end
    const u64 n_parts = (nq + JPM_PART_Q - 1) / JPM_PART_Q;
    u32 kept = 0;
    u32 loaded = ~0u;
    bool up = true;
    for (u64 part = blockIdx.x; part < n_parts; part += gridDim.x, up = !up)
    {
        const u64 q0 = part * JPM_PART_Q;
        u64 hits = 0; // bit 4 * k + b: row b of this thread's k-th quad of the part
        for (u32 si = 0; si < n_slices; ++si)
        {
            const u32 sl = up ? si : n_slices - 1 - si;
            const u32 slice_lo = sl * JPL_SLICE_BITS;
            const u32 slice_bits = dense_bits - slice_lo < JPL_SLICE_BITS ? dense_bits - slice_lo : JPL_SLICE_BITS;
            if (loaded != sl)
            {
                __syncthreads(); // every wave has finished probing the slice that is about to be replaced
                const u32 n_words = (slice_bits + 31) / 32;
                const u32 * src = pf_words + slice_lo / 32;
                for (u32 w = threadIdx.x * 4; w < n_words; w += 1024 * 4) // (slices start on 16-byte boundaries: JPL_SLICE_BITS % 128 == 0)
                {
                    if (w + 4 <= n_words)
                        *(v4u *)(jpl_bits + w) = *(const v4u *)(src + w);
                    else
                        for (u32 x = w; x < n_words; ++x)
                            jpl_bits[x] = src[x];
                }
                __syncthreads();
                loaded = sl;
            }
            const bool last = si + 1 == n_slices;
            auto found_in_slice = [&](u32 k) -> u32 {
                const u32 rel = k - slice_lo;
                const bool in = k != 0 && rel < slice_bits;
                const u32 r = in ? rel : 0;
                const u32 bit = (jpl_bits[r >> 5] >> (r & 31)) & 1u;
                return in ? bit : 0u;
            };
            constexpr int U = 4;
#pragma unroll 1
            for (u32 kb = 0; kb < JPM_QPT; kb += U) // (unrolled, the sixteen loads are hoisted together and spill)
            {
                v4u kk[U];
                u32 nm[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                {
                    const u64 q = q0 + (u64)(kb + u) * 1024 + threadIdx.x;
                    const u64 qc = q < nq ? q : nq - 1;
                    kk[u] = *((const v4u *)keys + qc); // plain loads: the other slices of this part find the lines in L2 / Infinity Cache
                    nm[u] = (HAS_NULL && last) ? *((const u32 *)null_map + qc) : 0u;
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                {
                    const u64 q = q0 + (u64)(kb + u) * 1024 + threadIdx.x;
                    const u32 k4[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w};
                    u32 h = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        h |= found_in_slice(k4[b]) << b;
                    hits |= (u64)h << (4 * (kb + u));
                    if (last)
                    {
                        const u32 hb = (u32)(hits >> (4 * (kb + u))) & 15u;
                        u32 acc = 0;
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                        {
                            const bool ok = !HAS_NULL || ((nm[u] >> (8 * b)) & 0xffu) == 0; // HashJoinMethodsImpl.h:451-452
                            const u32 f = ok ? (((hb >> b) & 1u) | ((k4[b] == 0 && has_zero) ? 1u : 0u)) : 0u; // the zero key lives out of line (HashTable.h:874-898)
                            acc |= f << (8 * b);
                        }
                        acc = anti ? acc ^ 0x01010101u : acc; // :515-519, :535-536
                        if (q < nq)
                        {
                            kept += (u32)__popc(acc);
                            __builtin_nontemporal_store(acc, (u32 *)filter + q);
                        }
                    }
                }
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (u32)(n & 3))
    {
        // the last n % 4 rows, against the whole bitmap in global memory
        const u64 i = nq * 4 + threadIdx.x;
        const u32 k = keys[i];
        const bool ok = !(HAS_NULL && null_map[i]);
        const bool found = ok && (k == 0 ? has_zero != 0 : (k < dense_bits && ((pf_words[k >> 5] >> (k & 31)) & 1u) != 0));
        const u8 f = anti ? !found : found;
        filter[i] = f;
        kept += f;
    }
    join_add_kept(ctrl, kept);
}

// probe pass 2b: where does max_joined_block_rows cut?  offsets are inclusive cumulative counts.
__global__ void k_join_cut(const u64 * __restrict__ offsets, u64 n, u64 max_rows, JoinCtrl * __restrict__ ctrl)
{
    if (blockIdx.x != 0 || threadIdx.x != 0)
        return;
    u64 consumed = n;
    if (max_rows != 0 && n > 0)
    {
        // the loop stops BEFORE row i when the offset after row i-1 is already >= max (HashJoinMethodsImpl.h:436-444):
        // consumed = 1 + (first index whose inclusive offset >= max), capped at n
        u64 lo = 0, hi = n; // first idx in [0,n) with offsets[idx] >= max_rows
        while (lo < hi)
        {
            const u64 mid = (lo + hi) / 2;
            if (offsets[mid] >= max_rows)
                hi = mid;
            else
                lo = mid + 1;
        }
        if (lo < n)
            consumed = lo + 1;
    }
    ctrl->consumed = consumed;
    ctrl->n_out = consumed ? offsets[consumed - 1] : 0;
}

// probe pass 3: write the appended right row ids (streams counts/offsets/values; touches rowids only for duplicate keys)
__global__ __launch_bounds__(JT) void k_join_emit(JoinTable t, int variant, const u64 * __restrict__ val_of_left,
                                                  const u32 * __restrict__ counts, const u64 * __restrict__ offsets, u64 consumed,
                                                  u64 * __restrict__ right_rowid)
{
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < consumed; i += (u64)gridDim.x * JT)
    {
        const u32 c = counts[i];
        if (c == 0)
            continue;
        const u64 base = offsets[i] - c;
        const u64 v = val_of_left[i];
        if (v == NO_ROW || variant == PV_ANTI_LEFT)
        {
            right_rowid[base] = NO_ROW; // default row (addNotFoundRow -> insertDefault)
            continue;
        }
        if (jv_single(v))
        {
            right_rowid[base] = v;
            continue;
        }
        const u64 * run = jv_run(t, v);
        for (u32 k = 0; k < c; ++k)
            right_rowid[base + k] = run[k];
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// Table capacity for `rows` build rows: a power of two with load factor in (0.35, 0.7].  Denser than the reference's
// 0.5 cap on purpose: the table is immutable after the build and a 1e7-row build then needs 2^24 cells (134 MB of keys),
// which stays resident in the 256 MB Infinity Cache, where 2^25 cells would not.
__global__ __launch_bounds__(JT) void k_join_mark_used(const u64 * __restrict__ rowid, u64 n, const u64 * __restrict__ block_base, u64 n_blocks, u64 total_rows,
                                                       u8 * __restrict__ used)
{
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
    {
        const u64 r = rowid[i];
        const u64 b = r >> 32;
        if (r == NO_ROW || b >= n_blocks)
            continue; // the default row of a LEFT / FULL miss
        const u64 f = join_flat_row(block_base, n_blocks, r);
        if (f < total_rows)
            used[f] = 1; // plain store: every writer stores the same value
    }
}

// RIGHT ANTI: a probe emits nothing; the left row that won a key's bid (the first to find it, over all blocks) marks every right row of
// that key as used -- once per key, however many left rows find it (used_flags.setUsed(find_result), HashJoinMethodsImpl.h:515-519)
__global__ __launch_bounds__(JT) void k_join_mark_used_keys(JoinTable t, const u32 * __restrict__ slot_of_left, const u64 * __restrict__ val_of_left, u64 n, u64 seq_base,
                                                            const u64 * __restrict__ block_base, u64 n_blocks, u64 total_rows, u8 * __restrict__ used)
{
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
    {
        const u32 slot = slot_of_left[i];
        if (slot == NO_SLOT || t.used_by[slot] != seq_base + i)
            continue;
        const u64 v = val_of_left[i];
        auto mark = [&](u64 r) {
            if ((r >> 32) < n_blocks)
            {
                const u64 f = join_flat_row(block_base, n_blocks, r);
                if (f < total_rows)
                    used[f] = 1;
            }
        };
        jv_for_each_row(t, v, jv_rows(t, v, slot), mark);
    }
}

// NotJoinedHash (src/Interpreters/HashJoin/HashJoin.cpp:1280-1420): the build rows no probe row ever matched -- rows whose key was
// NULL or whose ON mask was 0 included (they were never inserted, so they are never used) -- as (block << 32 | row) ids
__global__ __launch_bounds__(JT) void k_join_unused_flags(const u8 * __restrict__ used, u64 n, u32 * __restrict__ flag)
{
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
        flag[i] = used[i] ? 0u : 1u;
}

__global__ __launch_bounds__(JT) void k_join_unused_emit(const u32 * __restrict__ flag, const u64 * __restrict__ pos, u64 n, const u64 * __restrict__ block_base,
                                                         u64 n_blocks, u64 * __restrict__ out)
{
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
    {
        if (!flag[i])
            continue;
        u64 lo = 0, hi = n_blocks - 1; // largest block with base <= i
        while (lo < hi)
        {
            const u64 mid = (lo + hi + 1) >> 1;
            if (block_base[mid] <= i)
                lo = mid;
            else
                hi = mid - 1;
        }
        out[pos[i]] = (lo << 32) | (i - block_base[lo]);
    }
}

static u64 jpow2_ceil(u64 x)
{
    u64 p = 256;
    while (p < x)
        p <<= 1;
    return p;
}

extern "C" int chgpu_join_create(chgpu_ctx * ctx, int key_type, int kind, int strictness, int any_take_last_row,
                                 uint64_t size_hint, chgpu_join ** out)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    (void)size_hint;
    CHGPU_REQUIRE(ctx && out, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(chgpu_type_is_int(key_type),
                  CHGPU_ERR_NOT_IMPLEMENTED, "join key type %d: CPU path", key_type);
    CHGPU_REQUIRE(kind >= CHGPU_JOIN_INNER && kind <= CHGPU_JOIN_FULL, CHGPU_ERR_NOT_IMPLEMENTED, "join kind %d: CPU path", kind);
    CHGPU_REQUIRE(kind != CHGPU_JOIN_FULL || strictness == CHGPU_STRICT_ALL, CHGPU_ERR_NOT_IMPLEMENTED,
                  "FULL joins are carried for strictness ALL only (FULL ANY is a TODO in the reference too, HashJoinMethodsImpl.h:511-514): CPU path");
    CHGPU_REQUIRE(strictness >= CHGPU_STRICT_ANY && strictness <= CHGPU_STRICT_ANTI, CHGPU_ERR_NOT_IMPLEMENTED, "join strictness %d: CPU path", strictness);
    CHGPU_REQUIRE(!((strictness == CHGPU_STRICT_SEMI || strictness == CHGPU_STRICT_ANTI) && kind != CHGPU_JOIN_LEFT && kind != CHGPU_JOIN_RIGHT), CHGPU_ERR_NOT_IMPLEMENTED,
                  "only SEMI / ANTI LEFT and RIGHT are valid (joinDispatch.h:52-64)");
    chgpu_join * j = new chgpu_join();
    j->ctx = ctx;
    j->key_type = key_type;
    j->kind = kind;
    j->strictness = strictness;
    j->any_take_last_row = any_take_last_row ? 1 : 0;
    chgpu_ctx_retain(ctx);
    *out = j;
    return CHGPU_OK;
}

extern "C" int chgpu_join_free(chgpu_join * j)
{
    ChgpuDeviceGuard _dev_guard(j ? j->ctx : nullptr);
    if (!j)
        return CHGPU_OK;
    for (auto & b : j->blocks)
    {
        chgpu_pool_free(j->ctx, b.keys, b.keys_class);
        chgpu_pool_free(j->ctx, b.valid, b.valid_class);
    }
    if (j->table_mem)
        chgpu_pool_free(j->ctx, j->table_mem, j->table_class);
    if (j->used)
        chgpu_pool_free(j->ctx, j->used, j->used_class);
    if (j->block_base_dev)
        chgpu_pool_free(j->ctx, j->block_base_dev, j->base_class);
    if (j->ks_pf)
        chgpu_pool_free(j->ctx, j->ks_pf, j->ks_class);
    if (j->dm_rows)
        chgpu_pool_free(j->ctx, j->dm_rows, j->dm_class);
    if (j->key_stats)
        chgpu_pool_free(j->ctx, j->key_stats, j->key_stats_class);
    chgpu_ctx * ctx = j->ctx;
    delete j;
    chgpu_ctx_release(ctx);
    return CHGPU_OK;
}

extern "C" int chgpu_join_add_block(chgpu_join * j, const chgpu_col * key_col, const chgpu_col * null_map, const chgpu_col * join_mask,
                                    uint32_t * block_index_out)
{
    ChgpuDeviceGuard _dev_guard(j ? j->ctx : nullptr);
    CHGPU_REQUIRE(j && key_col, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(!j->finished && !j->build_closed, CHGPU_ERR_LOGICAL, "addBlockToJoin after onBuildPhaseFinish");
    CHGPU_REQUIRE(key_col->type == j->key_type, CHGPU_ERR_BAD_ARGUMENTS, "key column has type %d, expected %d", key_col->type, j->key_type);
    CHGPU_REQUIRE(key_col->rows < 0xFFFFFFFFull, CHGPU_ERR_TOO_MANY_ROWS, "Too many rows in right table block for HashJoin: %llu", (unsigned long long)key_col->rows); // HashJoin.cpp:563-564
    CHGPU_REQUIRE(j->blocks.size() < 0x7FFFFFFFull, CHGPU_ERR_TOO_MANY_ROWS, "too many right blocks"); // bit 63 of a row id tags packed multi-row values
    if (null_map)
        CHGPU_REQUIRE(null_map->type == CHGPU_U8 && null_map->rows == key_col->rows, CHGPU_ERR_SIZES_MISMATCH, "null map size mismatch");
    if (join_mask)
        CHGPU_REQUIRE(join_mask->type == CHGPU_U8 && join_mask->rows == key_col->rows, CHGPU_ERR_SIZES_MISMATCH, "join mask size mismatch");
    chgpu_ctx * ctx = j->ctx;
    BuildBlock b;
    b.rows = key_col->rows;
    b.base = j->total_rows;
    if (b.rows)
    {
        // the right block stays alive for the join's lifetime (data->blocks, HashJoin.cpp:656-658): keep its keys in HBM
        CHGPU_TRY(chgpu_pool_alloc(ctx, b.rows * sizeof(u64), (void **)&b.keys, &b.keys_class));
        if (null_map || join_mask)
        {
            const int rc = chgpu_pool_alloc(ctx, b.rows, (void **)&b.valid, &b.valid_class);
            if (rc != CHGPU_OK)
            {
                chgpu_pool_free(ctx, b.keys, b.keys_class);
                return rc;
            }
        }
        if (!j->key_stats)
        {
            int rc = chgpu_pool_alloc(ctx, 256, (void **)&j->key_stats, &j->key_stats_class);
            if (rc == CHGPU_OK && hipMemsetAsync(j->key_stats, 0, 32, ctx->stream) != hipSuccess)
                rc = chgpu_set_error(CHGPU_ERR_DEVICE, "memset failed");
            if (rc != CHGPU_OK)
            {
                chgpu_pool_free(ctx, b.keys, b.keys_class);
                if (b.valid)
                    chgpu_pool_free(ctx, b.valid, b.valid_class);
                return rc;
            }
        }
        hipLaunchKernelGGL(k_join_stage_keys, dim3(chgpu_grid_for(ctx, b.rows, JT, 8)), dim3(JT), 0, ctx->stream, (const void *)key_col->data, key_col->type,
                           null_map ? (const u8 *)null_map->data : nullptr, join_mask ? (const u8 *)join_mask->data : nullptr, b.rows, b.keys, b.valid, j->key_stats);
        ctx->counters[6] += 1;
        // the caller may free its columns right after this call returns.  Columns that own pool memory go back to this context's pool, whose
        // reuse is ordered on this stream behind the staging kernel; anything else (wrapped caller memory, views) may be released or
        // overwritten by means this stream does not order: wait.
        auto pooled_here = [&](const chgpu_col * c) { return !c || (c->owns && c->ctx == ctx); };
        if (!pooled_here(key_col) || !pooled_here(null_map) || !pooled_here(join_mask))
            CHGPU_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (block_index_out)
        *block_index_out = (u32)j->blocks.size();
    j->blocks.push_back(b);
    j->total_rows += b.rows;
    ctx->counters[2] += b.rows;
    return CHGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// The join's two-level partition, shared by the slice build, the LDS-staged probe, both sides of the radix join and (first level only)
// the region probe: k_rp_hist_wide + scan + k_rp_scatter into P contiguous first-level partitions, then k_rp_tilesort_keys of every
// tile by its second-level bucket.  What is partitioned picks both tiles: a key that carries an 8-byte word (build rows: row id or
// payload) stages 16 bytes per row in LDS, a key alone (probe keys) 8.
// ---------------------------------------------------------------------------------------------
static constexpr u32 jpart_scatter_tile(bool word) { return word ? 8192 : 12288; }
static constexpr u32 jpart_sort_tile(bool word) { return word ? 8192 : 16384; }

static u32 jceil_log2(u64 x)
{
    u32 lg = 0;
    while ((1ull << lg) < x)
        ++lg;
    return lg;
}

// The partition functors of a table placed by intHash64: the first level is the top bits of the home slot, the second level the next
// bits, counted from the first-level partition of the tile's first key
struct JoinRegionFn
{
    u64 mask;
    u32 shift;
    __device__ __forceinline__ u32 operator()(u64 key) const { return (u32)((dev_intHash64(key) & mask) >> shift); }
};
struct JoinBucket2Fn
{
    u64 mask;
    u32 shift2; // home slot -> second-level region (slice) number
    u32 lg_p2;  // slices per first-level partition
    __device__ __forceinline__ u32 operator()(u64 key, u64 first) const
    {
        const u32 r = (u32)((dev_intHash64(key) & mask) >> shift2), r0 = (u32)((dev_intHash64(first) & mask) >> shift2) >> lg_p2 << lg_p2;
        return r - r0; // 0 .. 2 * P2 - 1 for the tile's own and the next first-level partition (keys sort by partition, so r >= r0)
    }
};

// Carves 256-byte aligned pieces off one scratch allocation.  A caller runs its carve twice, over base 0 to size the allocation and
// over the allocation itself, so the size cannot drift from the layout.
struct JoinCarve
{
    uintptr_t at;
    template <typename T> T * take(u64 count)
    {
        T * r = (T *)at;
        at += (count * sizeof(T) + 255) / 256 * 256;
        return r;
    }
    // the last piece of a layout: nothing follows it, so its end is not padded
    template <typename T> T * last(u64 count)
    {
        T * r = (T *)at;
        at += count * sizeof(T);
        return r;
    }
};

// The buffers of one partition (words1 / words2: nullptr without a word; keys2 / words2 / tidx: nullptr for the first level alone)
struct JoinPart
{
    u32 * counts;          // [P * G] keys per (partition, workgroup)
    u64 * offsets;         // [P * G] their exclusive scan: where each run starts
    u64 * total;           // the scan's total
    void * tmp;            // the scan's temporaries
    u64 * keys1, * words1; // the first level
    u64 * keys2, * words2; // the second level: every tile sorted by bucket
    unsigned short * tidx; // [tiles][PB + 1] where each bucket's run starts inside its tile
};
// What `carve(JoinCarve &)` takes, off the context's scratch: carved over base 0 for the size, then over the scratch itself
template <typename Fn>
static int join_carve_scratch(chgpu_ctx * ctx, Fn && carve)
{
    JoinCarve size{0};
    carve(size);
    void * scratch = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, size.at, &scratch));
    JoinCarve c{(uintptr_t)scratch};
    carve(c);
    return CHGPU_OK;
}
// The scratch of one plan: an 8-word header, then what `carve(JoinCarve &)` takes.  -> *header, zeroed on the stream.
template <typename Fn>
static int join_scratch(chgpu_ctx * ctx, u64 ** header, Fn && carve)
{
    CHGPU_TRY(join_carve_scratch(ctx, [&](JoinCarve & c) {
        *header = c.take<u64>(8);
        carve(c);
    }));
    CHGPU_HIP(hipMemsetAsync(*header, 0, 64, ctx->stream));
    return CHGPU_OK;
}

// PB: second-level buckets per tile (0: the first level alone)
static JoinPart join_part_carve(JoinCarve & c, u64 n, u32 G, u32 P, u32 PB, bool word)
{
    const u64 m = (u64)P * G, tile = jpart_sort_tile(word), tiles = (n + tile - 1) / tile;
    JoinPart b{};
    b.counts = c.take<u32>(m);
    b.offsets = c.take<u64>(m + 1);
    b.total = c.take<u64>(1);
    b.tmp = c.take<char>(chgpu_scan_tmp_bytes(m));
    b.keys1 = c.take<u64>(n + RP_SCATTER_SLACK);
    if (word)
        b.words1 = c.take<u64>(n + RP_SCATTER_SLACK);
    if (PB)
    {
        b.keys2 = c.take<u64>(tiles * tile + 8); // (+ slack: an empty run at the very end of the last tile is addressed one row past it)
        if (word)
            b.words2 = c.take<u64>(tiles * tile + 8);
        b.tidx = c.take<unsigned short>(tiles * (PB + 1) + 8);
    }
    return b;
}

// The first level: keys (and words) -> b.keys1 (b.words1) in P contiguous partitions; b.offsets[p * G + g] is where workgroup g's run
// of partition p starts
template <bool WORD, typename Fn1>
static int join_partition(chgpu_ctx * ctx, const JoinPart & b, const u64 * keys, const u64 * words, u64 n, u32 P, Fn1 fn1)
{
    constexpr u32 TILE = jpart_scatter_tile(WORD);
    const u32 G = (u32)ctx->num_cus;
    const u64 m = (u64)P * G;
    const u64 rows_per_wg = ((n + G - 1) / G + 63) / 64 * 64;
    hipLaunchKernelGGL((k_rp_hist_wide<u64, Fn1>), dim3(G), dim3(RP_THREADS), 0, ctx->stream, keys, n, rows_per_wg, P, b.counts, fn1);
    CHGPU_TRY(chgpu_scan_exclusive_u32_u64(ctx, b.counts, b.offsets, m, b.total, b.tmp, chgpu_scan_tmp_bytes(m)));
    const size_t lds = rp_scatter_lds_bytes(TILE, P, 8, WORD);
    auto scat = k_rp_scatter<TILE, u64, WORD, Fn1>;
    CHGPU_HIP(hipFuncSetAttribute((const void *)scat, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(scat, dim3(G), dim3(RP_THREADS), lds, ctx->stream, keys, words, n, rows_per_wg, P, (const u64 *)b.offsets, b.keys1, b.words1, fn1);
    return CHGPU_OK;
}

// Both levels: the first, then every tile of b.keys1 (b.words1) sorted into PB buckets -> b.keys2 (b.words2) and b.tidx.  A tile that
// spans more than two first-level partitions raises *stray.
template <bool WORD, typename Fn1, typename Fn2>
static int join_partition2(chgpu_ctx * ctx, const JoinPart & b, const u64 * keys, const u64 * words, u64 n, u32 P, Fn1 fn1, u32 PB, Fn2 fn2, u32 * stray)
{
    CHGPU_TRY(join_partition<WORD>(ctx, b, keys, words, n, P, fn1));
    constexpr u32 TILE = jpart_sort_tile(WORD);
    const u32 G = (u32)ctx->num_cus;
    const u64 rows_per_wg = ((n + G - 1) / G + TILE - 1) / TILE * TILE;
    const size_t lds = (size_t)TILE * (WORD ? 16 : 8) + (size_t)(PB + 1) * 8 + 64;
    auto sortk = k_rp_tilesort_keys<TILE, Fn2, RP_THREADS, WORD>;
    CHGPU_HIP(hipFuncSetAttribute((const void *)sortk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(sortk, dim3(G), dim3(RP_THREADS), lds, ctx->stream, (const u64 *)b.keys1, n, rows_per_wg, PB, b.keys2, b.tidx, fn2, stray, (const u64 *)b.words1,
                       b.words2);
    return CHGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// Unique-key build at streaming speed (the primary-key build sides of star joins).  The generic build claims one cell per row with a
// device-scope CAS -- ~2e10/s whatever the bandwidth: 0.66 ms for 1e7 rows.  Here the build rows are partitioned down to table slices
// of 4096 cells with the same two passes as the LDS-staged probe (k_rp_hist_wide + k_rp_scatter into 64 partitions, k_rp_tilesort_keys
// inside them, the row id travelling as the word), every slice is then built by ONE workgroup in LDS (LDS compare-and-swap, linear
// probing inside the slice) and written out as one contiguous 64 KiB piece.  A row whose chain runs past its slice's end goes to a
// short overflow list that a last kernel inserts the generic way.  A duplicate key raises a flag and the generic build runs instead.
// ---------------------------------------------------------------------------------------------
// The probe's functors under names of their own: the build's partition kernels then carry these names in their symbols, which is how
// profiles/summarize_pmc.py tells them from the probe's.
struct JoinSliceFn1 : JoinRegionFn
{
};
struct JoinSliceFn2 : JoinBucket2Fn
{
};
static constexpr u32 JBS_LG_CELLS = 12, JBS_CELLS = 1u << JBS_LG_CELLS, JBS_TILE = jpart_sort_tile(true), JBS_LG_P1 = 6, JBS_THREADS = 512, JBS_MAX_OVERFLOW = 1u << 20;

// The slice geometry of a table of `cap` cells: JSL_P1 first-level partitions of 2^lg_p2 slices each, PB second-level buckets per tile
// (a tile may span two first-level partitions).  fits: between one slice and 128 per partition.
struct JoinSliceGeom
{
    bool fits;
    u32 lg_cap, lg_p2, P1, PB;
};
static JoinSliceGeom join_slice_geom(u64 cap)
{
    JoinSliceGeom g{};
    g.lg_cap = jceil_log2(cap);
    g.fits = g.lg_cap >= JBS_LG_CELLS + JBS_LG_P1 && g.lg_cap <= JBS_LG_CELLS + JBS_LG_P1 + 7;
    g.lg_p2 = g.fits ? g.lg_cap - JBS_LG_CELLS - JBS_LG_P1 : 0;
    g.P1 = 1u << JBS_LG_P1;
    g.PB = 2u << g.lg_p2;
    return g;
}

__global__ __launch_bounds__(256) void k_join_iota(u64 * __restrict__ out, u64 n)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
        out[i] = i; // row id of block 0: (0 << 32) | row
}

// ---------------------------------------------------------------------------------------------
// The work unit of the two-level partition, for the kernels that take a table slice by slice (k_join_build_slices, k_join_probe_lds):
// slice r2 = second-level region p2 of first-level partition p1; its rows are among [rb, re) of the partitioned array, tile-sorted by
// second-level bucket; its cells start at cell `slice` of the table.  Both kernels use one geometry: JBS_CELLS cells per slice, JSL_P1
// first-level partitions.
// ---------------------------------------------------------------------------------------------
static constexpr u32 JSL_P1 = 1u << JBS_LG_P1;
struct SliceUnit
{
    u32 p1, p2;
    u64 rb, re, slice;
};

// s_off[p] = where first-level partition p starts (s_off[JSL_P1] = n); visible after the caller's next barrier
__device__ __forceinline__ void jpart_stage_offsets(u64 * s_off, const u64 * __restrict__ off1, u32 G, u64 n, u32 threads)
{
    for (u32 p = threadIdx.x; p <= JSL_P1; p += threads)
        s_off[p] = p < JSL_P1 ? off1[(u64)p * G] : n;
}

// The workgroup takes the next unit number off the counter; `meanwhile` runs between the two barriers (what a kernel has to clear for
// the new unit).  A number >= JSL_P1 << lg_p2: no unit is left (every workgroup reaches this exit).  The caller tests that itself and
// then decodes the number with slice_unit: with the test in here, returned as a bool, both kernels needed 8-10 more VGPRs, and
// k_join_probe_lds<false> lost an occupancy step.
template <typename Fn>
__device__ __forceinline__ u32 slice_unit_claim(u32 * unit_ctr, Fn && meanwhile)
{
    __shared__ u32 sh_unit;
    __syncthreads(); // everyone is done with the previous unit (its number and what it kept in LDS)
    if (threadIdx.x == 0)
        sh_unit = atomicAdd(unit_ctr, 1u);
    meanwhile();
    __syncthreads();
    return sh_unit;
}
__device__ __forceinline__ SliceUnit slice_unit(u32 r2, const u64 * s_off, u32 lg_p2)
{
    SliceUnit u;
    u.p1 = r2 >> lg_p2;
    u.p2 = r2 & ((1u << lg_p2) - 1);
    u.rb = s_off[u.p1];
    u.re = s_off[u.p1 + 1];
    u.slice = (u64)r2 * JBS_CELLS;
    return u;
}

// The unit's run inside tile `tile` (of TILE rows, sorted by k_rp_tilesort_keys into PB buckets): rows [start, start + len) of the tile.
// A tile's buckets count from the first-level partition that owns the tile's first row: the largest p with s_off[p] <= row0 (empty
// partitions share their start with the next one: the largest such p is the owner).  A tile spanning three partitions has no bucket for
// this unit (len = 0): k_rp_tilesort_keys raised the stray flag and the host discards the run.
__device__ __forceinline__ void jpart_tile_run(const u64 * s_off, const SliceUnit & u, u32 tile, u32 TILE, const unsigned short * __restrict__ tile_index, u32 PB, u32 & start,
                                               u32 & len)
{
    const u64 row0 = (u64)tile * TILE;
    u32 lo = 0, hi = JSL_P1 - 1;
    while (lo < hi)
    {
        const u32 mid = (lo + hi + 1) >> 1;
        if (s_off[mid] <= row0)
            lo = mid;
        else
            hi = mid - 1;
    }
    const u32 bucket = (u.p1 - lo) * (PB >> 1) + u.p2;
    start = len = 0;
    if (bucket < PB)
    {
        const u32 a = tile_index[(u64)tile * (PB + 1) + bucket], b = tile_index[(u64)tile * (PB + 1) + bucket + 1];
        start = a;
        len = b - a;
    }
}

// A wave's tiles are tile0, tile0 + stride, ...: lane k fetches the run of the k-th of them, `left` in all (one round trip for up to 64
// tiles instead of one per tile) ...
__device__ __forceinline__ void jpart_lane_runs(const u64 * s_off, const SliceUnit & u, u32 tile0, u32 stride, u32 left, u32 TILE, const unsigned short * __restrict__ tile_index,
                                                u32 PB, u32 & st_l, u32 & ln_l)
{
    st_l = ln_l = 0;
    const u32 lane = threadIdx.x & 63;
    if (lane < left)
        jpart_tile_run(s_off, u, tile0 + lane * stride, TILE, tile_index, PB, st_l, ln_l);
}
// ... and every lane reads run k out of lane k: its first row in the partitioned array and its length (k >= nk: no rows, at a valid address)
__device__ __forceinline__ void jpart_run_of(u32 st_l, u32 ln_l, u32 k, u32 nk, u32 tile0, u32 stride, u32 TILE, u64 & row, u32 & len)
{
    const u32 kk = k < nk ? k : nk - 1;
    const u32 st = (u32)__builtin_amdgcn_readlane((int)st_l, (int)kk);
    len = k < nk ? (u32)__builtin_amdgcn_readlane((int)ln_l, (int)kk) : 0;
    row = (u64)(tile0 + kk * stride) * TILE + st;
}

// Claims a cell for `want` in a slice staged in LDS, whose key words lie STRIDE words apart: compare-and-swap, linear probing from cell c
// up to cell `end`.  c is left at the cell that answered; what happens to a chain that runs out of cells is the caller's policy.
enum { LDS_CLAIMED, LDS_DUPLICATE, LDS_RAN_OUT };
template <u32 STRIDE>
__device__ __forceinline__ int lds_claim(u64 * keyw, u32 & c, u32 end, u64 want)
{
    while (c < end)
    {
        const u64 old = atomicCAS((unsigned long long *)&keyw[STRIDE * c], 0ull, (unsigned long long)want);
        if (old == 0)
            return LDS_CLAIMED;
        if (old == want)
            return LDS_DUPLICATE;
        ++c;
    }
    return LDS_RAN_OUT;
}

// flags[0] = a duplicate key was met, [1] = overflow entries, [2] = the overflow list was too short
__global__ __launch_bounds__(JBS_THREADS) void k_join_build_slices(JoinTable t, const u64 * __restrict__ keys2, const u64 * __restrict__ rids2, u64 n, const u64 * __restrict__ off1, u32 G,
                                                                   u32 lg_p2, const unsigned short * __restrict__ tile_index, u32 * __restrict__ unit_ctr, u32 * __restrict__ flags,
                                                                   u64 * __restrict__ ovf_keys, u64 * __restrict__ ovf_rids)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char jbs_lds[];
    u64 * ck = (u64 *)jbs_lds;       // [JBS_CELLS] keys
    u64 * cv = ck + JBS_CELLS;       // [JBS_CELLS] row ids
    constexpr u32 NW = JBS_THREADS / 64;
    __shared__ u64 s_off[JSL_P1 + 1];
    const u32 PB = 2u << lg_p2;
    jpart_stage_offsets(s_off, off1, G, n, JBS_THREADS);
    const u32 lane = threadIdx.x & 63;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 mask = t.capacity - 1;
    u32 inserted = 0;
    u64 my_max = 0;
    bool dup = false;
    for (;;)
    {
        // (the first barrier in there: the previous slice has been written out)
        const u32 r2 = slice_unit_claim(unit_ctr, [&] {
            for (u32 c = threadIdx.x; c < JBS_CELLS; c += JBS_THREADS)
                ck[c] = 0;
        });
        if (r2 >= (JSL_P1 << lg_p2))
            break;
        const SliceUnit u = slice_unit(r2, s_off, lg_p2);
        if (u.rb != u.re)
        {
            const u32 t_lo = (u32)(u.rb / JBS_TILE), t_hi = (u32)((u.re - 1) / JBS_TILE);
            for (u32 tile = t_lo + wave; tile <= t_hi; tile += NW)
            {
                const u64 row0 = (u64)tile * JBS_TILE;
                u32 a, len;
                jpart_tile_run(s_off, u, tile, JBS_TILE, tile_index, PB, a, len);
                for (u32 o = lane; o < len; o += 64)
                {
                    const u64 key = keys2[row0 + a + o], rid = rids2[row0 + a + o];
                    my_max = key > my_max ? key : my_max;
                    if (key == 0)
                    {
                        // the zero key lives out of line (cell `capacity`)
                        if (atomicExch(&t.ctrl->has_zero, 1u) == 0)
                        {
                            t.kv[2 * t.capacity + 1] = rid;
                            ++inserted;
                        }
                        else
                            dup = true;
                        continue;
                    }
                    u32 c = (u32)((dev_intHash64(key) & mask) - u.slice);
                    const int claim = lds_claim<1>(ck, c, JBS_CELLS, key);
                    if (claim == LDS_CLAIMED)
                    {
                        cv[c] = rid; // nobody reads it before the barrier below
                        ++inserted;
                    }
                    else if (claim == LDS_DUPLICATE)
                        dup = true;
                    else
                    {
                        // the chain leaves the slice: the row goes to the overflow list
                        const u32 at = atomicAdd(&flags[1], 1u);
                        if (at < JBS_MAX_OVERFLOW)
                        {
                            ovf_keys[at] = key;
                            ovf_rids[at] = rid;
                        }
                        else
                            flags[2] = 1;
                    }
                }
            }
        }
        __syncthreads();
        // the slice goes out as it lies: 4096 {key, row id} cells = 64 KiB, contiguous
        for (u32 c = threadIdx.x; c < JBS_CELLS; c += JBS_THREADS)
        {
            const u64 k = ck[c];
            __builtin_nontemporal_store(jv2{k, k ? cv[c] : 0ull}, (jv2 *)(t.kv + 2 * (u.slice + c)));
        }
    }
    const u32 tot = wave_reduce_add_u32(inserted);
    my_max = wave_reduce_max_u64(my_max);
    if (lane == 0 && tot)
        atomicAdd(&t.ctrl->n_keys, (unsigned long long)tot);
    if (lane == 0 && my_max)
        atomicMax(&t.ctrl->max_key, (unsigned long long)my_max);
    if (dup)
        flags[0] = 1;
}

// the overflow list through the generic claim (after every slice has been written)
__global__ __launch_bounds__(JT) void k_join_insert_pairs(JoinTable t, const u64 * __restrict__ keys, const u64 * __restrict__ rids, const u32 * __restrict__ flags)
{
    const u32 n = flags[1] < JBS_MAX_OVERFLOW ? flags[1] : JBS_MAX_OVERFLOW;
    u32 claims = 0;
    bool dup = false;
    for (u32 i = blockIdx.x * JT + threadIdx.x; i < n; i += gridDim.x * JT)
    {
        bool claimed = false;
        const u32 slot = jt_emplace(t, keys[i], claimed);
        if (claimed)
        {
            t.kv[2 * (u64)slot + 1] = rids[i];
            ++claims;
        }
        else
            dup = true;
    }
    if (claims)
        atomicAdd(&t.ctrl->n_keys, (unsigned long long)claims);
    if (dup)
        ((u32 *)flags)[0] = 1;
}

// Why a plan that ran declined its result (the `debug` option prints these): bit set of the flags its kernels raised
enum : u32
{
    JOIN_DECLINED_STRAY = 1,         // a tile spanned three first-level partitions, or a chain ran past the staged window
    JOIN_DECLINED_DUP = 2,           // a duplicate build key
    JOIN_DECLINED_OVERFLOW_FULL = 4, // the slice build's overflow list was too short
};
static void join_debug_declined(const chgpu_ctx * ctx, const char * what, u32 declined)
{
    if (!chgpu_opt(ctx, "debug", 0))
        return;
    fprintf(stderr, "chgpu: %s declined:%s%s%s%s\n", what, declined ? "" : " shape", (declined & JOIN_DECLINED_STRAY) ? " stray" : "",
            (declined & JOIN_DECLINED_DUP) ? " dup" : "", (declined & JOIN_DECLINED_OVERFLOW_FULL) ? " overflow_list_full" : "");
}

// -> CHGPU_OK: the table is built (unique keys) and its used_by words are cleared; NOT_IMPLEMENTED: shape does not fit or a duplicate
// key exists (the caller runs the generic build, which zeroes the table itself).  *declined: the flags that made a run decline (0: it did not run); *overflow: the rows
// that went through the overflow list.
static int join_build_slices(chgpu_join * j, JoinTable & t, u32 * declined, u64 * overflow)
{
    chgpu_ctx * ctx = j->ctx;
    const bool off = chgpu_opt(ctx, "tune_join_no_slice_build", 0) != 0;
    const u64 n = j->total_rows, cap = t.capacity;
    // the slices are written out whole: only the control block and the zero key's cell need clearing first (ahead of the shape test, as
    // ever: a declined build costs these two small memsets)
    CHGPU_HIP(hipMemsetAsync(t.ctrl, 0, (size_t)((char *)t.kv - (char *)t.ctrl), ctx->stream));
    CHGPU_HIP(hipMemsetAsync(t.kv + 2 * cap, 0, 16, ctx->stream));
    const JoinSliceGeom geom = join_slice_geom(cap);
    if (off || j->blocks.size() != 1 || j->blocks[0].valid || n < (1u << 20) || n + JBS_TILE + RP_SCATTER_SLACK >= (1ull << 32) || !geom.fits
        || ((uintptr_t)j->blocks[0].keys % 16) != 0)
        return CHGPU_ERR_NOT_IMPLEMENTED;
    const u32 lg_cap = geom.lg_cap, lg_p2 = geom.lg_p2, P1 = geom.P1, PB = geom.PB;
    const JoinSliceFn1 fn1{{cap - 1, lg_cap - JBS_LG_P1}};
    const JoinSliceFn2 fn2{{cap - 1, JBS_LG_CELLS, lg_p2}};
    const u32 G = (u32)ctx->num_cus;
    u64 * flags_dev, * rid0, * ovf_keys, * ovf_rids; // flags_dev: [2] unit counter | stray flag, [3..4] flags[0..3]
    JoinPart part;
    CHGPU_TRY(join_scratch(ctx, &flags_dev, [&](JoinCarve & c) {
        rid0 = c.take<u64>(n);
        ovf_keys = c.take<u64>(JBS_MAX_OVERFLOW);
        ovf_rids = c.take<u64>(JBS_MAX_OVERFLOW);
        part = join_part_carve(c, n, G, P1, PB, true);
    }));
    u32 * unit_ctr = (u32 *)(flags_dev + 2), * stray = unit_ctr + 1, * flags = (u32 *)(flags_dev + 3);
    hipLaunchKernelGGL(k_join_iota, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, rid0, n);
    CHGPU_TRY(join_partition2<true>(ctx, part, j->blocks[0].keys, rid0, n, P1, fn1, PB, fn2, stray));
    {
        const size_t lds = (size_t)JBS_CELLS * 16;
        CHGPU_HIP(hipFuncSetAttribute((const void *)k_join_build_slices, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_join_build_slices, dim3(2 * G), dim3(JBS_THREADS), lds, ctx->stream, t, (const u64 *)part.keys2, (const u64 *)part.words2, n,
                           (const u64 *)part.offsets, G, lg_p2, (const unsigned short *)part.tidx, unit_ctr, flags, ovf_keys, ovf_rids);
    }
    hipLaunchKernelGGL(k_join_insert_pairs, dim3(64), dim3(JT), 0, ctx->stream, t, (const u64 *)ovf_keys, (const u64 *)ovf_rids, (const u32 *)flags);
    ctx->counters[6] += 7;
    CHGPU_HIP(hipGetLastError());
    u64 back[3];
    CHGPU_TRY(chgpu_read_back(ctx, flags_dev + 2, back, 24));
    const u32 stray_v = (u32)(back[0] >> 32), dup_v = (u32)back[1], too_long = (u32)back[2];
    *declined = (stray_v ? JOIN_DECLINED_STRAY : 0) | (dup_v ? JOIN_DECLINED_DUP : 0) | (too_long ? JOIN_DECLINED_OVERFLOW_FULL : 0);
    *overflow = back[1] >> 32;
    if (stray_v || dup_v || too_long)
        return CHGPU_ERR_NOT_IMPLEMENTED;
    // (unique keys: first_row / cnt are only read for cells that hold several rows -- there are none)
    if (t.used_by)
        CHGPU_HIP(hipMemsetAsync(t.used_by, 0xFF, (cap + 1) * 8, ctx->stream));
    return CHGPU_OK;
}

static int join_build_table(chgpu_join * j);
static u64 join_capacity_for(const chgpu_ctx * ctx, u64 rows)
{
    const u32 cap_shift = (u32)chgpu_opt(ctx, "tune_join_cap_shift", 1);
    return jpow2_ceil(rows + rows * 3 / 7 + 1) << cap_shift;
}

// IJoin::onBuildPhaseFinish: the right side is complete.  The hash table is built by the first consumer that needs it (joinBlock, the
// key count, non-joined rows ...): the fused probe of a large unique-key build side never does -- it joins partition by partition
// (join_probe_agg_radix).  CHGPU_TUNE_JOIN_EAGER_BUILD=1 builds here, as before.
extern "C" int chgpu_join_finish_build(chgpu_join * j)
{
    ChgpuDeviceGuard _dev_guard(j ? j->ctx : nullptr);
    CHGPU_REQUIRE(j, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    const bool eager = chgpu_opt(j->ctx, "tune_join_eager_build", 0) != 0;
    j->build_closed = true;
    return eager ? join_build_table(j) : CHGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// The table build: a plan (what the table holds), a layout (where), one of two builders (the inserts and the memsets they need) and one
// finish (everything after the inserts).
// ---------------------------------------------------------------------------------------------
enum JoinPfKind
{
    JOIN_PF_NONE,
    JOIN_PF_HASH,  // 16 bits per build row, one multiplicative hash (exact all the same when the largest key is below the bit count)
    JOIN_PF_DENSE, // a larger build side of narrow keys: one bit per key value up to the largest key
};
struct JoinBuildPlan
{
    bool maps_all;  // CSR arrays: every row of a key is kept
    bool flagged;   // a cell remembers the left row that consumed it
    bool take_last; // ANY keeps the last row of a key, not the first
    u64 cap, cells; // cells = cap + 1: the zero key's cell sits behind the table
    JoinPfKind pf;
    u64 pf_bits;
};

// The prefilter's kind and size.  The one device pass of the plan: the dense kind needs the largest staged key.
static int join_choose_prefilter(chgpu_join * j, JoinBuildPlan * p)
{
    chgpu_ctx * ctx = j->ctx;
    p->pf = JOIN_PF_NONE;
    p->pf_bits = 1ull << 16;
    while (p->pf_bits < 16 * j->total_rows && p->pf_bits < (1ull << 25))
        p->pf_bits <<= 1;
    if (chgpu_opt(ctx, "tune_join_no_prefilter", 0))
        return CHGPU_OK;
    if (p->pf_bits >= 16 * j->total_rows)
    {
        p->pf = JOIN_PF_HASH;
        return CHGPU_OK;
    }
    // A larger build side of narrow DENSE keys (a filtered dimension table joined on its surrogate key: SSB's customer, 6 M of the keys
    // 1..30 M) still gets the exact bitmap if max_key + 1 bits fit the 4 MiB limit: the misses of the probe then stop at a bitmap that
    // lives in L2 / Infinity Cache instead of costing one HBM sector each.
    if (chgpu_type_size(j->key_type) > 4 || chgpu_opt(ctx, "tune_join_no_dense_prefilter", 0))
        return CHGPU_OK;
    void * scratch0 = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, 256, &scratch0));
    CHGPU_HIP(hipMemsetAsync(scratch0, 0, 8, ctx->stream));
    for (const BuildBlock & b : j->blocks)
        if (b.rows)
            hipLaunchKernelGGL(k_join_max_key, dim3(chgpu_grid_for(ctx, b.rows, JT, 4)), dim3(JT), 0, ctx->stream, (const u64 *)b.keys, b.rows, (unsigned long long *)scratch0);
    u64 mk = 0;
    CHGPU_TRY(chgpu_read_back(ctx, scratch0, &mk, sizeof(mk)));
    if (mk < (1ull << 25))
    {
        p->pf = JOIN_PF_DENSE;
        p->pf_bits = 1ull << 16;
        while (p->pf_bits <= mk)
            p->pf_bits <<= 1;
    }
    return CHGPU_OK;
}

static int join_plan_build(chgpu_join * j, JoinBuildPlan * p)
{
    // joinDispatch.h:30-68: MapsAll for every ALL join and for every RIGHT join (RIGHT ANY / SEMI / ANTI keep all rows of a key); a cell
    // remembers the left row that consumed it for INNER ANY and for RIGHT ANY / SEMI / ANTI (setUsedOnce / the per-key flag)
    p->maps_all = j->strictness == CHGPU_STRICT_ALL || j->kind == CHGPU_JOIN_RIGHT;
    p->flagged = (j->kind == CHGPU_JOIN_INNER && j->strictness == CHGPU_STRICT_ANY) || (j->kind == CHGPU_JOIN_RIGHT && j->strictness != CHGPU_STRICT_ALL);
    p->take_last = !p->maps_all && j->any_take_last_row;
    // load factor in (0.175, 0.35]: a probe then resolves at its home cell nearly always (1.1 cells per hit, 1.3 per miss, against 1.75 / 3.6
    // at 0.6).  Measured at C4: build 1.00 -> 0.90 ms (fewer retried claims), probe 3.40 -> 2.26 ms region-partitioned, 4.83 -> 3.39 ms
    // one-pass.  The table is immutable after the build and 288 GB of HBM make the doubled footprint (512 MB of cells for 1e7 rows) cheap.
    p->cap = join_capacity_for(j->ctx, j->total_rows);
    CHGPU_REQUIRE(p->cap + 1 < 0xFFFFFFFFull, CHGPU_ERR_NOT_IMPLEMENTED, "build side of %llu rows exceeds the 32-bit cell index", (unsigned long long)j->total_rows);
    p->cells = p->cap + 1;
    return join_choose_prefilter(j, p);
}

// The table's memory: the only place that knows the offsets.  Over base 0 the pointers are the offsets and `bytes` sizes the allocation.
struct JoinTableLayout
{
    JoinTable t;
    size_t bytes;
};
static JoinTableLayout join_table_layout(const JoinBuildPlan & p, u64 total_rows, uintptr_t base = 0)
{
    JoinCarve c{base};
    JoinTable t{};
    t.ctrl = (JoinCtrl *)c.take<char>(256);
    t.kv = c.take<u64>(p.cells * 2);
    t.first_row = c.take<u64>(p.cells);
    t.cnt = p.maps_all ? c.take<u32>(p.cells) : nullptr;
    t.start = p.maps_all ? c.take<u64>(p.cells) : nullptr;
    t.used_by = p.flagged ? c.take<u64>(p.cells) : nullptr;
    t.rowids = p.maps_all ? c.take<u64>(total_rows) : nullptr;
    t.pf = p.pf != JOIN_PF_NONE ? c.take<u32>(p.pf_bits / 32) : nullptr;
    c.take<char>(256); // (slack behind the last array)
    t.capacity = p.cap;
    t.pf_mask = p.pf_bits - 1;
    return {t, (size_t)(c.at - base)};
}

// What the generic inserts leave for the CSR fill, and the fill's own temporaries
struct JoinBuildScratch
{
    u32 * slot_of_row; // [total_rows + 1] the cell every build row went to
    u32 * cursor;      // [cells]
    u64 * total;
    void * tmp;        // the scan's temporaries
    size_t tmp_bytes;
};
static JoinBuildScratch join_build_carve(JoinCarve & c, u64 total_rows, u64 cells)
{
    JoinBuildScratch s{};
    s.slot_of_row = c.take<u32>(total_rows + 1);
    s.cursor = c.take<u32>(cells);
    s.total = c.take<u64>(1);
    s.tmp_bytes = chgpu_scan_tmp_bytes(cells);
    s.tmp = c.last<char>(s.tmp_bytes);
    return s;
}
// (asked for by the generic inserts and again by the finish, which also follows the slice build: the second request finds the scratch
//  large enough and does nothing)
static int join_build_scratch(chgpu_join * j, const JoinBuildPlan & p, JoinBuildScratch * s)
{
    return join_carve_scratch(j->ctx, [&](JoinCarve & c) { *s = join_build_carve(c, j->total_rows, p.cells); });
}

// One device-scope claim per row over a zeroed table.  first_row starts at ~0 for atomicMin, 0 for atomicMax(+1).
static int join_build_generic(chgpu_join * j, const JoinBuildPlan & p)
{
    chgpu_ctx * ctx = j->ctx;
    const JoinTable & t = j->t;
    CHGPU_HIP(hipMemsetAsync(t.ctrl, 0, (size_t)((char *)t.first_row - (char *)t.ctrl), ctx->stream)); // ctrl + {key, value} cells
    CHGPU_HIP(hipMemsetAsync(t.first_row, p.take_last ? 0x00 : 0xFF, p.cells * 8, ctx->stream));
    if (p.maps_all)
        CHGPU_HIP(hipMemsetAsync(t.cnt, 0, p.cells * 4, ctx->stream));
    if (p.flagged)
        CHGPU_HIP(hipMemsetAsync(t.used_by, 0xFF, p.cells * 8, ctx->stream));
    JoinBuildScratch s;
    CHGPU_TRY(join_build_scratch(j, p, &s));
    for (size_t bi = 0; bi < j->blocks.size(); ++bi)
    {
        const BuildBlock & b = j->blocks[bi];
        if (!b.rows)
            continue;
        hipLaunchKernelGGL(k_join_insert, dim3(chgpu_grid_for(ctx, b.rows, JT, 8)), dim3(JT), 0, ctx->stream, t, (const u64 *)b.keys, (const u8 *)b.valid, b.rows,
                           (u64)bi, p.maps_all ? 1 : 0, p.take_last ? 1 : 0, s.slot_of_row + b.base);
        ctx->counters[6] += 1;
    }
    return CHGPU_OK;
}

// First flat row of every right block -> dst[max(blocks, 1)]: row ids (block << 32 | row) -> position in payload columns glued over all
// blocks.  `host` is the copy's source: the caller keeps it until it has waited for the stream.
static size_t join_block_bases_bytes(const chgpu_join * j) { return (j->blocks.empty() ? 1 : j->blocks.size()) * sizeof(u64); }
static int join_upload_block_bases(const chgpu_join * j, u64 * dst, std::vector<u64> & host)
{
    host.assign(join_block_bases_bytes(j) / sizeof(u64), 0);
    for (size_t b = 0; b < j->blocks.size(); ++b)
        host[b] = j->blocks[b].base;
    CHGPU_HIP(hipMemcpyAsync(dst, host.data(), host.size() * sizeof(u64), hipMemcpyHostToDevice, j->ctx->stream));
    return CHGPU_OK;
}

// ALL over duplicate keys: the rows of every key gathered into its CSR run -> j->inserted
static int join_fill_csr(chgpu_join * j, const JoinBuildPlan & p, const JoinBuildScratch & s)
{
    chgpu_ctx * ctx = j->ctx;
    const JoinTable & t = j->t;
    CHGPU_TRY(chgpu_scan_exclusive_u32_u64(ctx, t.cnt, t.start, p.cells, s.total, s.tmp, s.tmp_bytes));
    CHGPU_HIP(hipMemsetAsync(s.cursor, 0, p.cells * 4, ctx->stream));
    for (size_t bi = 0; bi < j->blocks.size(); ++bi)
    {
        const BuildBlock & b = j->blocks[bi];
        if (!b.rows)
            continue;
        hipLaunchKernelGGL(k_join_fill, dim3(chgpu_grid_for(ctx, b.rows, JT, 8)), dim3(JT), 0, ctx->stream, t, (const u32 *)(s.slot_of_row + b.base), b.rows, (u64)bi, s.cursor);
        ctx->counters[6] += 1;
    }
    hipLaunchKernelGGL(k_join_root_first, dim3(chgpu_grid_for(ctx, p.cells, JT, 8)), dim3(JT), 0, ctx->stream, t);
    ctx->counters[6] += 1;
    return chgpu_read_back(ctx, s.total, &j->inserted, sizeof(u64));
}

// Everything after the inserts of either builder: the used flags and block bases the probes need, then -- the one decision about it --
// what is left to do to the cells, from whether any key got a second row and which builder ran.
static int join_finish_table(chgpu_join * j, const JoinBuildPlan & p, bool sliced)
{
    chgpu_ctx * ctx = j->ctx;
    const JoinTable & t = j->t;
    JoinBuildScratch s;
    CHGPU_TRY(join_build_scratch(j, p, &s));
    if (jf_track_used(j))
    {
        void * um = nullptr;
        CHGPU_TRY(chgpu_pool_alloc(ctx, j->total_rows + 64, &um, &j->used_class));
        j->used = (u8 *)um;
        CHGPU_HIP(hipMemsetAsync(j->used, 0, j->total_rows + 64, ctx->stream));
    }
    // (uploaded here so that the read-back below -- which waits for the stream -- also covers this copy out of a host temporary)
    std::vector<u64> bases;
    void * bm = nullptr;
    CHGPU_TRY(chgpu_pool_alloc(ctx, join_block_bases_bytes(j), &bm, &j->base_class));
    j->block_base_dev = (u64 *)bm;
    CHGPU_TRY(join_upload_block_bases(j, j->block_base_dev, bases));
    // did any key get a second row?  (one small read-back; the common primary-key build then skips four passes over the table)
    JoinCtrl c;
    CHGPU_TRY(chgpu_read_back(ctx, t.ctrl, &c, sizeof(c)));
    const bool unique = c.pad == 0;
    j->unique_keys = unique;
    if (!unique)
    {
        hipLaunchKernelGGL(k_join_merge_claims, dim3(chgpu_grid_for(ctx, p.cells, JT, 8)), dim3(JT), 0, ctx->stream, t, p.maps_all ? 1 : 0, p.take_last ? 1 : 0);
        ctx->counters[6] += 1;
    }
    if (p.maps_all && !unique)
        CHGPU_TRY(join_fill_csr(j, p, s));
    else if (p.maps_all)
        j->inserted = c.n_keys;
    if (sliced && unique)
    {
        // the slices carry their final values: only a prefilter is left to fill
        if (t.pf)
        {
            hipLaunchKernelGGL(k_join_pf_fill, dim3(chgpu_grid_for(ctx, j->blocks[0].rows, JT, 8)), dim3(JT), 0, ctx->stream, t, (const u64 *)j->blocks[0].keys, j->blocks[0].rows);
            ctx->counters[6] += 1;
        }
    }
    else if (!unique || t.pf)
    {
        // (without duplicates and without a prefilter there is nothing to finalise: the value word of an empty cell is never read)
        hipLaunchKernelGGL(k_join_finalize_values, dim3(chgpu_grid_for(ctx, p.cells, JT, 8)), dim3(JT), 0, ctx->stream, t, p.maps_all ? 1 : 0, p.take_last ? 1 : 0, unique ? 1 : 0);
        ctx->counters[6] += 1;
    }
    CHGPU_HIP(hipGetLastError());
    // unique keys: nothing after the inserts touches the control block -- the read-back above already holds the final key count, the
    // largest key and the zero-key flag (one host synchronisation per build instead of three)
    if (!unique)
        CHGPU_TRY(chgpu_read_back(ctx, t.ctrl, &c, sizeof(c)));
    j->n_keys = c.n_keys;
    j->max_key = c.max_key;
    j->has_zero = c.has_zero != 0;
    j->finished = true;
    return CHGPU_OK;
}

static int join_build_table(chgpu_join * j)
{
    if (j->finished)
        return CHGPU_OK;
    j->build_closed = true;
    chgpu_ctx * ctx = j->ctx;
    JoinBuildPlan p;
    CHGPU_TRY(join_plan_build(j, &p));
    void * m = nullptr;
    CHGPU_TRY(chgpu_pool_alloc(ctx, join_table_layout(p, j->total_rows).bytes, &m, &j->table_class)); // pooled: no hipMalloc/hipFree per join
    j->table_mem = m;
    j->t = join_table_layout(p, j->total_rows, (uintptr_t)m).t;
    if (j->t.pf)
        CHGPU_HIP(hipMemsetAsync(j->t.pf, 0, p.pf_bits / 8, ctx->stream));
    // unique keys, one right block: the table slices are built in LDS and written out whole (join_build_slices).  Anything else -- or a
    // duplicate key met on the way -- takes the generic build.
    u32 slices_declined = 0;
    u64 slices_overflow = 0;
    const int fast = join_build_slices(j, j->t, &slices_declined, &slices_overflow);
    if (fast != CHGPU_OK && fast != CHGPU_ERR_NOT_IMPLEMENTED)
        return fast;
    const bool sliced = fast == CHGPU_OK;
    if (!sliced && slices_declined)
        join_debug_declined(ctx, "join build slices", slices_declined);
    if (!sliced)
        CHGPU_TRY(join_build_generic(j, p));
    CHGPU_TRY(join_finish_table(j, p, sliced));
    if (chgpu_opt(ctx, "debug", 0))
    {
        const JoinKeySet ks = join_key_set(j);
        fprintf(stderr, "chgpu: join build plan=%s rows=%llu cap=%llu overflow=%llu pf=%s unique=%d\n", sliced ? "slices" : "generic", (unsigned long long)j->total_rows,
                (unsigned long long)p.cap, (unsigned long long)slices_overflow, ks.dense ? "dense" : ks.pf ? "hash" : "none", j->unique_keys ? 1 : 0);
    }
    return CHGPU_OK;
}

// The temporaries of chgpu_join_non_joined_rows over n build rows (pool memory, not the context's scratch)
struct JoinUnusedScratch
{
    u32 * flag; // [n] the row was not used
    u64 * pos;  // [n] the flags' exclusive scan
    u64 * total;
    void * tmp; // the scan's temporaries
    size_t bytes;
};
static JoinUnusedScratch join_unused_carve(JoinCarve c, u64 n)
{
    const uintptr_t base = c.at;
    JoinUnusedScratch u{};
    u.flag = c.take<u32>(n);
    u.pos = c.take<u64>(n);
    u.total = c.take<u64>(1);
    u.tmp = c.last<char>(chgpu_scan_tmp_bytes(n));
    u.bytes = c.at - base;
    return u;
}

/* IJoin::getNonJoinedBlocks (src/Interpreters/IJoin.h:133-134; NotJoinedHash, HashJoin.cpp:1280-1420) for RIGHT / FULL joins: after the
   last joinBlock, the build rows no left row matched, as (block << 32 | row) ids in insertion order; the caller gathers the right
   columns there and pads the left columns with defaults. */
extern "C" int chgpu_join_non_joined_rows(chgpu_join * j, chgpu_col ** right_rowid_u64, uint64_t * rows_out)
{
    ChgpuDeviceGuard _dev_guard(j ? j->ctx : nullptr);
    CHGPU_REQUIRE(j && right_rowid_u64 && rows_out, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(jf_track_used(j), CHGPU_ERR_LOGICAL, "non-joined rows exist for RIGHT / FULL joins only");
    if (!j->finished)
        CHGPU_TRY(join_build_table(j));
    chgpu_ctx * ctx = j->ctx;
    const u64 n = j->strictness == CHGPU_STRICT_SEMI ? 0 : j->total_rows; // JoinCommon::hasNonJoinedBlocks (JoinUtils.cpp:634-638): none for SEMI
    chgpu_col * out = nullptr;
    u64 total = 0;
    if (n)
    {
        const size_t b_tmp = chgpu_scan_tmp_bytes(n);
        void * mem = nullptr;
        size_t mem_class = 0;
        CHGPU_TRY(chgpu_pool_alloc(ctx, join_unused_carve(JoinCarve{0}, n).bytes, &mem, &mem_class));
        const JoinUnusedScratch u = join_unused_carve(JoinCarve{(uintptr_t)mem}, n);
        u32 * flag = u.flag;
        u64 * pos = u.pos, * total_dev = u.total;
        void * tmp = u.tmp;
        const u32 grid = chgpu_grid_for(ctx, n, JT, 8);
        hipLaunchKernelGGL(k_join_unused_flags, dim3(grid), dim3(JT), 0, ctx->stream, (const u8 *)j->used, n, flag);
        int rc = chgpu_scan_exclusive_u32_u64(ctx, flag, pos, n, total_dev, tmp, b_tmp);
        if (rc == CHGPU_OK)
            rc = chgpu_read_back(ctx, total_dev, &total, sizeof(total));
        if (rc == CHGPU_OK)
            rc = chgpu_col_new(ctx, CHGPU_U64, total, &out);
        if (rc == CHGPU_OK && total)
            hipLaunchKernelGGL(k_join_unused_emit, dim3(grid), dim3(JT), 0, ctx->stream, (const u32 *)flag, (const u64 *)pos, n, (const u64 *)j->block_base_dev,
                               (u64)j->blocks.size(), (u64 *)out->data);
        ctx->counters[6] += 2;
        chgpu_pool_free(ctx, mem, mem_class);
        if (rc != CHGPU_OK)
            return rc;
        CHGPU_HIP(hipGetLastError());
    }
    else
        CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, 0, &out));
    *right_rowid_u64 = out;
    *rows_out = total;
    return CHGPU_OK;
}

__global__ __launch_bounds__(JT) void k_join_flatten(const u64 * __restrict__ rowid, u64 n, const u64 * __restrict__ block_base, u64 n_blocks, u64 * __restrict__ out)
{
    for (u64 i = (u64)blockIdx.x * JT + threadIdx.x; i < n; i += (u64)gridDim.x * JT)
    {
        const u64 r = rowid[i];
        out[i] = (r == NO_ROW || (r >> 32) >= n_blocks) ? NO_ROW : join_flat_row(block_base, n_blocks, r);
    }
}

extern "C" int chgpu_join_flatten_rowids(chgpu_join * j, const chgpu_col * rowids, chgpu_col ** flat)
{
    ChgpuDeviceGuard _dev_guard(j ? j->ctx : nullptr);
    CHGPU_REQUIRE(j && rowids && flat, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(chgpu_type_size(rowids->type) == 8, CHGPU_ERR_BAD_ARGUMENTS, "row ids must be a 64-bit column");
    chgpu_ctx * ctx = j->ctx;
    const u64 nb = j->blocks.size();
    // (a copy of its own in the scratch: the table, whose build uploads j->block_base_dev, may not exist yet and is not built for this)
    std::vector<u64> bases;
    void * scratch = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, join_block_bases_bytes(j), &scratch));
    CHGPU_TRY(join_upload_block_bases(j, (u64 *)scratch, bases));
    CHGPU_HIP(hipStreamSynchronize(ctx->stream)); // `bases` is a host temporary
    chgpu_col * out = nullptr;
    CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, rowids->rows, &out));
    if (rowids->rows)
    {
        hipLaunchKernelGGL(k_join_flatten, dim3(chgpu_grid_for(ctx, rowids->rows, JT, 8)), dim3(JT), 0, ctx->stream, (const u64 *)rowids->data, rowids->rows,
                           (const u64 *)scratch, nb, (u64 *)out->data);
        ctx->counters[6] += 1;
        // the scratch holding block_base is reused by the next call on this context
        CHGPU_HIP(hipStreamSynchronize(ctx->stream));
    }
    *flat = out;
    return CHGPU_OK;
}

extern "C" int chgpu_join_total_rows(chgpu_join * j, uint64_t * rows, uint64_t * keys)
{
    ChgpuDeviceGuard _dev_guard(j ? j->ctx : nullptr);
    CHGPU_REQUIRE(j, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    if (rows)
        *rows = j->total_rows; // IJoin::getTotalRowCount
    if (keys)
    {
        if (!j->finished)
            CHGPU_TRY(join_build_table(j));
        *keys = j->n_keys;
    }
    return CHGPU_OK;
}

// what a probe does per left row, from the join's kind and strictness
static int join_probe_variant(const chgpu_join * j)
{
    if (j->strictness == CHGPU_STRICT_ALL) return jf_left_kind(j) == CHGPU_JOIN_LEFT ? PV_ALL_LEFT : PV_ALL_INNER;
    if (jf_right_once(j)) return PV_ONCE_RIGHT;
    if (j->kind == CHGPU_JOIN_RIGHT) return PV_ANTI_RIGHT;
    if (j->strictness == CHGPU_STRICT_SEMI) return PV_SEMI_LEFT;
    if (j->strictness == CHGPU_STRICT_ANTI) return PV_ANTI_LEFT;
    return jf_left_kind(j) == CHGPU_JOIN_LEFT ? PV_ANY_LEFT : PV_ANY_INNER;
}

// LEFT SEMI / LEFT ANTI without right columns: the filter bytes and the number of kept rows alone
static int join_probe_filter_only(chgpu_join * j, const chgpu_col * key_col, const chgpu_col * null_map, bool anti, chgpu_col ** filter_out, uint64_t * n_out,
                                  uint64_t * n_left_consumed)
{
    chgpu_ctx * ctx = j->ctx;
    const u64 n = key_col->rows;
    JoinOutCol fcol;
    CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U8, n, &fcol.col));
    hipError_t e = hipMemsetAsync(&j->t.ctrl->n_out, 0, sizeof(u64), ctx->stream);
    const u8 * nm = null_map ? (const u8 *)null_map->data : nullptr;
    // dense 4-byte keys whose key set fits a few LDS slices: k_join_probe_filter_lds_multi (the tail of a bitmap beyond max_key is zero)
    const bool no_lds_filter = chgpu_opt(ctx, "tune_join_no_lds_filter", 0) != 0;
    const JoinKeySet ks = join_key_set(j);
    if (e == hipSuccess && !no_lds_filter && join_lds_filter_fits(ks, j->key_type, n, key_col->data, nm, JPL_SLICE_BITS, 4))
    {
        // one sweep, every part of the rows through all slices.  A single slice too: a kernel of its own for that case measured slower
        // (profiles/join_filter_single_vs_multi.json)
        const u32 slices = (u32)((ks.dense_bits + JPL_SLICE_BITS - 1) / JPL_SLICE_BITS);
        auto kern = null_map ? k_join_probe_filter_lds_multi<true> : k_join_probe_filter_lds_multi<false>;
        e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(JPL_SLICE_BITS / 8));
        if (e == hipSuccess)
            hipLaunchKernelGGL(kern, dim3((u32)ctx->num_cus), dim3(1024), (size_t)(JPL_SLICE_BITS / 8), ctx->stream, ks.pf, (u32)ks.dense_bits, slices,
                               anti ? 1 : 0, ks.has_zero ? 1 : 0, (const u32 *)key_col->data, nm, n, (u8 *)fcol.col->data, j->t.ctrl);
    }
    else if (e == hipSuccess)
    {
        auto kern = j->t.pf ? k_join_probe_filter<true> : k_join_probe_filter<false>;
        hipLaunchKernelGGL(kern, dim3(chgpu_grid_for(ctx, (n + JPF_R - 1) / JPF_R, JT, 8)), dim3(JT), 0, ctx->stream, j->t, anti ? 1 : 0, (const void *)key_col->data,
                           j->key_type, nm, n, (u8 *)fcol.col->data, j->t.ctrl);
    }
    if (e == hipSuccess)
    {
        ctx->counters[6] += 1;
        e = hipGetLastError();
    }
    JoinCtrl c;
    CHGPU_TRY(e == hipSuccess ? chgpu_read_back(ctx, j->t.ctrl, &c, sizeof(c)) : chgpu_set_error(CHGPU_ERR_DEVICE, "join probe launch: %s", hipGetErrorString(e)));
    j->left_seq += n;
    *filter_out = fcol.release();
    *n_out = c.n_out;
    *n_left_consumed = n;
    ctx->counters[3] += n;
    ctx->counters[4] += c.n_out;
    return CHGPU_OK;
}

// The per-left-row temporaries of chgpu_join_probe
struct JoinProbeScratch
{
    u32 * slot_of_left; // [n] the cell the row bid for
    u32 * counts;       // [n] joined rows per left row
    u64 * val_of_left;  // [n] the packed value of the matched cell
    u64 * total;
    void * tmp;         // the scan's temporaries
    size_t tmp_bytes;
};
static JoinProbeScratch join_probe_carve(JoinCarve & c, u64 n)
{
    JoinProbeScratch s{};
    s.slot_of_left = c.take<u32>(n);
    s.counts = c.take<u32>(n);
    s.val_of_left = c.take<u64>(n);
    s.total = c.take<u64>(1);
    s.tmp_bytes = chgpu_scan_tmp_bytes(n);
    s.tmp = c.last<char>(s.tmp_bytes);
    return s;
}

extern "C" int chgpu_join_probe(chgpu_join * j, const chgpu_col * key_col, const chgpu_col * null_map, uint64_t max_joined_block_rows,
                                chgpu_col ** filter_out, chgpu_col ** offsets_out, chgpu_col ** right_rowid_out, uint64_t * n_out,
                                uint64_t * n_left_consumed)
{
    ChgpuDeviceGuard _dev_guard(j ? j->ctx : nullptr);
    CHGPU_REQUIRE(j && key_col && n_out && n_left_consumed, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(key_col->type == j->key_type, CHGPU_ERR_BAD_ARGUMENTS, "left key column has type %d, expected %d", key_col->type, j->key_type);
    if (null_map)
        CHGPU_REQUIRE(null_map->type == CHGPU_U8 && null_map->rows == key_col->rows, CHGPU_ERR_SIZES_MISMATCH, "null map size mismatch");
    if (!j->finished)
        CHGPU_TRY(join_build_table(j));
    chgpu_ctx * ctx = j->ctx;
    const u64 n = key_col->rows;
    const bool need_filter = jf_need_filter(j), need_repl = jf_need_replication(j);
    CHGPU_REQUIRE(!need_filter || filter_out, CHGPU_ERR_BAD_ARGUMENTS, "this join variant produces a filter: filter_u8 must not be NULL");
    CHGPU_REQUIRE(!need_repl || offsets_out, CHGPU_ERR_BAD_ARGUMENTS, "this join variant produces offsets_to_replicate: offsets_u64 must not be NULL");
    CHGPU_REQUIRE(right_rowid_out || (need_filter && !need_repl && j->kind == CHGPU_JOIN_LEFT && (j->strictness == CHGPU_STRICT_SEMI || j->strictness == CHGPU_STRICT_ANTI)),
                  CHGPU_ERR_BAD_ARGUMENTS, "right_rowid_u64 may only be NULL for LEFT SEMI / LEFT ANTI (filter-only probe)");
    if (filter_out) *filter_out = nullptr;
    if (offsets_out) *offsets_out = nullptr;
    if (right_rowid_out) *right_rowid_out = nullptr;
    const int variant = join_probe_variant(j);
    if (!need_repl)
        max_joined_block_rows = 0; // the early stop only exists for need_replication (HashJoinMethodsImpl.h:434-444)

    if (n == 0)
    {
        if (need_filter) CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U8, 0, filter_out));
        if (need_repl) CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, 0, offsets_out));
        if (right_rowid_out) CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, 0, right_rowid_out));
        *n_out = 0;
        *n_left_consumed = 0;
        return CHGPU_OK;
    }

    if (!right_rowid_out)
        return join_probe_filter_only(j, key_col, null_map, variant == PV_ANTI_LEFT, filter_out, n_out, n_left_consumed);

    JoinProbeScratch s;
    CHGPU_TRY(join_carve_scratch(ctx, [&](JoinCarve & c) { s = join_probe_carve(c, n); }));
    u32 * slot_of_left = s.slot_of_left, * counts = s.counts;
    u64 * val_of_left = s.val_of_left;

    JoinOutCol filter_col, offsets_col, rowid_col;
    if (need_filter)
        CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U8, n, &filter_col.col));
    CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, n, &offsets_col.col));
    chgpu_col * const filter = filter_col.col, * const offsets = offsets_col.col;

    const u32 grid = chgpu_grid_for(ctx, n, JT, 8);
    const void * kp = key_col->data;
    const u8 * nm = null_map ? (const u8 *)null_map->data : nullptr;
    const u64 seq_base = j->left_seq;
    const bool bids = variant == PV_ANY_INNER || variant == PV_ONCE_RIGHT || variant == PV_ANTI_RIGHT;
    if (bids)
    {
        hipLaunchKernelGGL(j->t.pf ? k_join_probe_bid<true> : k_join_probe_bid<false>, dim3(grid), dim3(JT), 0, ctx->stream, j->t, kp, j->key_type, nm, n, seq_base, slot_of_left);
        ctx->counters[6] += 1;
    }
    hipLaunchKernelGGL(j->t.pf ? k_join_probe_count<true> : k_join_probe_count<false>, dim3(grid), dim3(JT), 0, ctx->stream, j->t, variant, kp, j->key_type, nm, n, seq_base,
                       bids ? 1 : 0, slot_of_left, val_of_left, counts, filter ? (u8 *)filter->data : nullptr);
    ctx->counters[6] += 1;
    if (variant == PV_ANTI_RIGHT)
    {
        hipLaunchKernelGGL(k_join_mark_used_keys, dim3(grid), dim3(JT), 0, ctx->stream, j->t, (const u32 *)slot_of_left, (const u64 *)val_of_left, n, seq_base,
                           (const u64 *)j->block_base_dev, (u64)j->blocks.size(), j->total_rows, j->used);
        ctx->counters[6] += 1;
    }
    CHGPU_TRY(chgpu_scan_inclusive_u32_u64(ctx, counts, (u64 *)offsets->data, n, s.total, s.tmp, s.tmp_bytes));
    hipLaunchKernelGGL(k_join_cut, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)offsets->data, n, (u64)max_joined_block_rows, j->t.ctrl);
    ctx->counters[6] += 1;
    JoinCtrl c;
    CHGPU_TRY(chgpu_read_back(ctx, j->t.ctrl, &c, sizeof(c)));
    CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, c.n_out, &rowid_col.col));
    chgpu_col * const rowid = rowid_col.col;
    if (c.n_out)
    {
        hipLaunchKernelGGL(k_join_emit, dim3(grid), dim3(JT), 0, ctx->stream, j->t, variant, (const u64 *)val_of_left, (const u32 *)counts,
                           (const u64 *)offsets->data, c.consumed, (u64 *)rowid->data);
        ctx->counters[6] += 1;
    }
    if (c.n_out && jf_track_used(j))
    {
        // used_flags.setUsed for every emitted right row (HashJoinMethodsImpl.h addFoundRowAll with flag_per_row)
        hipLaunchKernelGGL(k_join_mark_used, dim3(chgpu_grid_for(ctx, c.n_out, JT, 8)), dim3(JT), 0, ctx->stream, (const u64 *)rowid->data, (u64)c.n_out,
                           (const u64 *)j->block_base_dev, (u64)j->blocks.size(), j->total_rows, j->used);
        ctx->counters[6] += 1;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return chgpu_set_error(CHGPU_ERR_DEVICE, "join probe launch: %s", hipGetErrorString(e));
    // (the scratch buffers -- slot_of_left, counts -- are reused by the next call on this context, which launches on the same stream and so
    //  runs after the kernels above; chgpu_scratch drains the stream itself before it ever frees a buffer: no host synchronisation here)
    j->left_seq += c.consumed; // rows not consumed are resubmitted by the caller and bid again
    // outputs are cut to the consumed prefix (offsets_to_replicate->resize(i), filter.resize(i): :439-441)
    if (filter)
        filter->rows = c.consumed;
    offsets->rows = c.consumed;
    if (need_filter)
        *filter_out = filter_col.release();
    if (need_repl) // (otherwise the offsets only served the emit: they go with their holder)
        *offsets_out = offsets_col.release();
    *right_rowid_out = rowid_col.release();
    *n_out = c.n_out;
    *n_left_consumed = c.consumed;
    ctx->counters[3] += c.consumed;
    ctx->counters[4] += c.n_out;
    return CHGPU_OK;
}


// ---------------------------------------------------------------------------------------------
// Fused probe -> payload gather -> aggregate without key: joinBlock (HashJoinMethodsImpl.h:402-549) followed by
// AddedColumns' lazy gather (AddedColumns.cpp:39-131) and executeWithoutKeyImpl (Aggregator.cpp:1276-1321) in ONE pass over the
// left keys.  Nothing per left row is written: no counts, no packed values, no offsets_to_replicate, no row ids, no gathered column --
// the plan `SELECT count(), sum(right.v) FROM left JOIN right USING k` only ever needed two numbers.
// Every lane keeps R rows in flight (the table and payload reads are dependent random accesses); the {key, value} cell is fetched
// with one 16-byte load.
// ---------------------------------------------------------------------------------------------
// payload value at flat row f, widened to the 8-byte sum operand (integers sign/zero-extended, floats as Float64 bits)
__device__ __forceinline__ u64 jload_payload(const void * p, int type, u64 f)
{
    switch (type)
    {
        case CHGPU_I64: case CHGPU_U64: case CHGPU_F64: return ((const u64 *)p)[f];
        case CHGPU_U32: return ((const u32 *)p)[f];
        case CHGPU_I32: return (u64)(i64)((const i32 *)p)[f];
        case CHGPU_U16: return ((const u16 *)p)[f];
        case CHGPU_I16: return (u64)(i64)((const i16 *)p)[f];
        case CHGPU_U8: return ((const u8 *)p)[f];
        case CHGPU_I8: return (u64)(i64)((const i8 *)p)[f];
        default: return (u64)__double_as_longlong((double)((const float *)p)[f]); // CHGPU_F32
    }
}

template <bool PF, bool FLOAT>
__global__ __launch_bounds__(JT) void k_join_probe_agg(JoinTable t, int variant, const void * __restrict__ keys, int key_type, const u8 * __restrict__ null_map, u64 n,
                                                       const void * __restrict__ payload, int payload_type, const u64 * __restrict__ block_base, u64 n_blocks,
                                                       u64 * __restrict__ partials /* [grid][2] */)
{
    PfView pf{};
    if constexpr (PF)
        pf = jt_pf_view(t);
    constexpr int R = 4;
    u64 cnt = 0, isum = 0;
    double fsum = 0.0;
    auto add_row = [&](u64 rowid) {
        if (!payload)
            return;
        const u64 b = jload_payload(payload, payload_type, join_flat_row(block_base, n_blocks, rowid));
        if constexpr (FLOAT)
            fsum += __longlong_as_double((long long)b);
        else
            isum += b;
    };
    const u64 stride = (u64)gridDim.x * JT;
    for (u64 i0 = (u64)blockIdx.x * JT + threadIdx.x; i0 < n; i0 += stride * R)
    {
        u64 key[R];
        bool ok[R];
#pragma unroll
        for (int q = 0; q < R; ++q)
        {
            const u64 i = i0 + (u64)q * stride;
            ok[q] = i < n;
            key[q] = ok[q] ? jload_key(keys, key_type, i) : 0;
            ok[q] = ok[q] && !(null_map && null_map[i]);
        }
        u64 val[R];
        u32 slot[R];
#pragma unroll
        for (int q = 0; q < R; ++q)
            slot[q] = ok[q] ? jt_lookup<PF, true>(t, pf, key[q], val[q]) : NO_SLOT;
#pragma unroll
        for (int q = 0; q < R; ++q)
        {
            if (i0 + (u64)q * stride >= n)
                continue;
            if (!pv_account(variant, slot[q] != NO_SLOT, cnt))
                continue;
            const u32 c = jv_rows(t, val[q], slot[q]);
            cnt += c;
            jv_for_each_row(t, val[q], c, add_row);
        }
    }
    // one partial per workgroup
    u64 sbits = FLOAT ? (u64)__double_as_longlong(fsum) : isum;
    if (join_fold_workgroup<FLOAT>(cnt, sbits))
    {
        partials[2 * (u64)blockIdx.x] = cnt;
        partials[2 * (u64)blockIdx.x + 1] = sbits;
    }
}

template <bool FLOAT>
__global__ __launch_bounds__(64) void k_join_probe_agg_finish(const u64 * __restrict__ partials, u32 n_parts, u64 * __restrict__ out2)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    u64 c = 0, si = 0;
    double sf = 0.0;
    for (u32 p = 0; p < n_parts; ++p) // workgroup order: run-to-run reproducible Float64 sums
    {
        c += partials[2 * (u64)p];
        if constexpr (FLOAT)
            sf += __longlong_as_double((long long)partials[2 * (u64)p + 1]);
        else
            si += partials[2 * (u64)p + 1];
    }
    out2[0] = c;
    out2[1] = FLOAT ? (u64)__double_as_longlong(sf) : si;
}

// ---------------------------------------------------------------------------------------------
// The same fused probe for build sides far beyond a cache: the probe keys are first radix-partitioned by TABLE REGION (the top bits
// of their home slot) with the carried-tail partition of radix_partition.h, then every region's keys are probed by the workgroups of
// ONE XCD at a time, so the region's slice of the table (~1 MB) is fetched from HBM once and every further lookup is an L2 hit:
// the unpartitioned probe pays one random 64-byte HBM / Infinity-Cache transaction per key (3.8e10/s chip-wide over a 256 MB table)
// whatever the bandwidth.  Workgroup -> XCD placement is read from HW_REG_XCC_ID and only steers which queue a workgroup drains
// first; every workgroup ends up draining all eight queues, so the result never depends on it.
// ---------------------------------------------------------------------------------------------
static constexpr u32 JPR_CHUNK = 4096; // keys per work item
static constexpr u32 JPR_XCDS = 8;
static constexpr u32 JPR_MAX_REGIONS = 512;

// per XCD x: the chunks of regions x, x + 8, ... as one queue; qstart[x * (R/8 + 1) + i] = first chunk of its i-th region
__global__ void k_jp_queues(const u64 * __restrict__ offsets, u32 G, u32 R, u64 n, u32 * __restrict__ qstart, u32 * __restrict__ qctr)
{
    const u32 x = threadIdx.x;
    if (x >= JPR_XCDS)
        return;
    const u32 per = R / JPR_XCDS;
    u32 acc = 0;
    for (u32 i = 0; i < per; ++i)
    {
        const u32 r = x + i * JPR_XCDS;
        const u64 b = offsets[(u64)r * G], e = r + 1 < R ? offsets[(u64)(r + 1) * G] : n;
        qstart[x * (per + 1) + i] = acc;
        acc += (u32)((e - b + JPR_CHUNK - 1) / JPR_CHUNK);
    }
    qstart[x * (per + 1) + per] = acc;
    qctr[x] = 0;
}

// A primary-key build side probed for sum(payload): the payload of every cell's row is gathered ONCE into the cell's value word
// (a copy of the table: {key, widened payload}), so a hit needs no second random access -- and no access outside its table region:
// the row-id indirection into an 80 MB payload column cost 3.2 GB of line fetches per 1e8 probes and evicted the region's slice
// from the XCD's L2 while it was being probed (PMC FETCH_SIZE 9.6 GB per launch before, for 0.8 GB of keys and 0.5 GB of table).
__global__ __launch_bounds__(JT) void k_join_fuse_payload(JoinTable t, const void * __restrict__ payload, int payload_type, const u64 * __restrict__ block_base, u64 n_blocks,
                                                          u64 * __restrict__ kvp)
{
    for (u64 s = (u64)blockIdx.x * JT + threadIdx.x; s <= t.capacity; s += (u64)gridDim.x * JT)
    {
        const u64 k = t.kv[2 * s];
        u64 v = 0;
        if (jt_occupied(t, s))
            v = jload_payload(payload, payload_type, join_flat_row(block_base, n_blocks, t.kv[2 * s + 1]));
        *(jv2 *)(kvp + 2 * s) = jv2{k, v};
    }
}

// FUSED: t.kv points at such a {key, payload} copy (unique build keys): a hit adds the cell's second word
template <bool PF, bool FUSED = false>
__global__ __launch_bounds__(JT) void k_join_probe_agg_regions(JoinTable t, int variant, const u64 * __restrict__ keys, u64 n, const u64 * __restrict__ offsets, u32 G, u32 R,
                                                               const u32 * __restrict__ qstart, u32 * __restrict__ qctr, const void * __restrict__ payload, int payload_type,
                                                               const u64 * __restrict__ block_base, u64 n_blocks, unsigned long long * __restrict__ result2)
{
    PfView pf{};
    if constexpr (PF)
        pf = jt_pf_view(t);
    __shared__ u64 sh_begin, sh_end;
    __shared__ u32 sh_more;
    const u32 per = R / JPR_XCDS;
    // the queue tables and the region boundaries live in LDS: the lane that fetches a work item then makes no dependent global read
    __shared__ u32 s_qs[JPR_XCDS * (JPR_MAX_REGIONS / JPR_XCDS + 1)];
    __shared__ u64 s_roff[JPR_MAX_REGIONS + 1];
    for (u32 i = threadIdx.x; i < JPR_XCDS * (per + 1); i += JT)
        s_qs[i] = qstart[i];
    for (u32 r = threadIdx.x; r <= R; r += JT)
        s_roff[r] = r < R ? offsets[(u64)r * G] : n;
    const u32 xcc = __builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20) & (JPR_XCDS - 1); // HW_REG_XCC_ID[3:0]
    u64 cnt = 0, isum = 0;
    for (u32 dx = 0; dx < JPR_XCDS; ++dx)
    {
        const u32 x = (xcc + dx) & (JPR_XCDS - 1);
        const u32 * qs = s_qs + x * (per + 1);
        for (;;)
        {
            __syncthreads(); // the previous item's sh_* have been read by everyone
            if (threadIdx.x == 0)
            {
                const u32 c = atomicAdd(&qctr[x], 1u);
                u32 more = c < qs[per];
                if (more)
                {
                    u32 i = 0;
                    while (i + 1 < per && qs[i + 1] <= c)
                        ++i;
                    const u32 r = x + i * JPR_XCDS;
                    const u64 rb = s_roff[r], re = s_roff[r + 1];
                    const u64 b = rb + (u64)(c - qs[i]) * JPR_CHUNK;
                    sh_begin = b;
                    sh_end = b + JPR_CHUNK < re ? b + JPR_CHUNK : re;
                }
                sh_more = more;
            }
            __syncthreads();
            if (!sh_more)
                break; // every thread of the workgroup leaves this queue together; the counter only ever grows
            const u64 begin = sh_begin, end = sh_end;
            constexpr int RR = 8; // keys per lane and batch: their first cell reads (and then their payload reads) are all in flight together --
                                  // a lane that walks its keys one after the other has ONE random access outstanding
            static_assert(JPR_CHUNK == JT * RR * 2, "chunk = 256 threads x 2 batches x 8 keys");
            const u64 mask = t.capacity - 1;
#pragma unroll 1
            for (u32 batch = 0; batch < 2; ++batch)
            {
                u64 key[RR];
                jv2 cell[RR];
                u64 slot0[RR];
                bool in[RR];
#pragma unroll
                for (int q = 0; q < RR; ++q)
                {
                    const u64 i = begin + (u64)(batch * RR + q) * JT + threadIdx.x;
                    in[q] = i < end;
                    key[q] = in[q] ? __builtin_nontemporal_load(&keys[i]) : 0;
                }
#pragma unroll
                for (int q = 0; q < RR; ++q)
                {
                    slot0[q] = dev_intHash64(key[q]) & mask;
                    bool go = in[q] && key[q] != 0;
                    if constexpr (PF)
                        go = go && jt_pf_maybe(pf, key[q]);
                    cell[q] = go ? *(const jv2 *)(t.kv + 2 * slot0[q]) : jv2{0, 0};
                }
                u64 pay_row[RR];
                bool pay[RR];
#pragma unroll
                for (int q = 0; q < RR; ++q)
                {
                    pay[q] = false;
                    pay_row[q] = 0;
                    if (!in[q])
                        continue;
                    bool found = false;
                    u64 v = 0;
                    u32 sl = 0;
                    if (key[q] == 0)
                    {
                        found = t.ctrl->has_zero != 0;
                        sl = (u32)t.capacity;
                        v = found ? t.kv[2 * t.capacity + 1] : 0;
                    }
                    else if (cell[q].x == key[q])
                    {
                        found = true;
                        v = cell[q].y;
                        sl = (u32)slot0[q];
                    }
                    else if (cell[q].x != 0)
                    {
                        // the home cell belongs to another key: walk on (rare at the table's load factor; misses end at the first empty cell)
                        sl = jt_walk<true>(t.kv, t.capacity, key[q], (slot0[q] + 1) & mask, 1, v);
                        found = sl != NO_SLOT;
                    }
                    if (!pv_account(variant, found, cnt))
                        continue;
                    if constexpr (FUSED)
                    {
                        cnt += 1;
                        isum += v; // the value word IS the payload
                        continue;
                    }
                    if (jv_single(v))
                    {
                        // its payload read waits for the other keys' (below)
                        cnt += 1;
                        pay[q] = payload != nullptr;
                        pay_row[q] = join_flat_row(block_base, n_blocks, v);
                        continue;
                    }
                    const u32 c = jv_rows(t, v, sl);
                    cnt += c;
                    if (payload)
                        jv_for_each_row(t, v, c, [&](u64 r) { isum += jload_payload(payload, payload_type, join_flat_row(block_base, n_blocks, r)); });
                }
                // the single-row matches' payload reads, issued back to back
                if constexpr (!FUSED)
#pragma unroll
                    for (int q = 0; q < RR; ++q)
                        isum += pay[q] ? jload_payload(payload, payload_type, pay_row[q]) : 0;
            }
        }
    }
    // integer count and wrap-around sum: the order of the additions does not matter
    if (join_fold_workgroup<false>(cnt, isum))
    {
        atomicAdd(&result2[0], (unsigned long long)cnt);
        atomicAdd(&result2[1], (unsigned long long)isum);
    }
}

// -> CHGPU_OK with res[] filled, or CHGPU_ERR_NOT_IMPLEMENTED when this plan does not apply (the caller then runs the one-pass probe)
static int join_probe_agg_regions(chgpu_join * j, const chgpu_col * key_col, const chgpu_col * right_payload, int variant, u64 res[2], u32 * regions)
{
    chgpu_ctx * ctx = j->ctx;
    const u64 n = key_col->rows, cap = j->t.capacity;
    const bool off = chgpu_opt(ctx, "tune_join_no_regions", 0) != 0;
    const u64 min_rows = chgpu_opt(ctx, "tune_join_region_min_rows", (4ull << 20));
    // worth it when the table is far larger than the XCDs' L2s together (32 MB) and there are enough keys to pay two extra passes
    if (off || chgpu_type_size(j->key_type) != 8 || n < min_rows || n + RP_SCATTER_SLACK >= (1ull << 32) || cap * 16 < (64ull << 20) || ((uintptr_t)key_col->data % 16) != 0)
        return CHGPU_ERR_NOT_IMPLEMENTED;
    if (right_payload && chgpu_type_is_float(right_payload->type))
        return CHGPU_ERR_NOT_IMPLEMENTED; // a Float64 sum keeps the one-pass probe's fixed reduction order
    const u32 region_kib = (u32)chgpu_opt(ctx, "tune_join_region_kib", 1024);
    u32 R = 8;
    while (R < JPR_MAX_REGIONS && (cap * 16) / R > (u64)region_kib * 1024)
        R <<= 1;
    *regions = R;
    const JoinRegionFn fn{cap - 1, jceil_log2(cap) - jceil_log2(R)};
    const u32 G = (u32)ctx->num_cus;
    u64 * total_dev; // [2..3] the result
    u32 * qstart;
    JoinPart part;
    CHGPU_TRY(join_scratch(ctx, &total_dev, [&](JoinCarve & c) {
        qstart = c.take<u32>(JPR_XCDS * (R / JPR_XCDS + 1) + JPR_XCDS);
        part = join_part_carve(c, n, G, R, 0, false);
    }));
    u32 * qctr = qstart + JPR_XCDS * (R / JPR_XCDS + 1);
    const u64 * offsets = part.offsets, * pkeys = part.keys1;
    unsigned long long * result2 = (unsigned long long *)(total_dev + 2);
    // keys only, plain runs (k_rp_scatter; carried tails measured slower and wrote 1.26 GB for 0.8 GB of keys)
    CHGPU_TRY(join_partition<false>(ctx, part, (const u64 *)key_col->data, nullptr, n, R, fn));
    hipLaunchKernelGGL(k_jp_queues, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)offsets, G, R, n, qstart, qctr);
    const void * pp = right_payload ? right_payload->data : nullptr;
    const int pt = right_payload ? right_payload->type : CHGPU_U64;
    const u32 grid = (u32)ctx->num_cus * 4;
    auto probe = [&](auto kern, const JoinTable & t) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(JT), 0, ctx->stream, t, variant, (const u64 *)pkeys, n, (const u64 *)offsets, G, R, (const u32 *)qstart, qctr, pp, pt,
                           (const u64 *)j->block_base_dev, (u64)j->blocks.size(), result2);
    };
    const bool no_fuse = chgpu_opt(ctx, "tune_join_no_fused_payload", 0) != 0;
    if (j->unique_keys && right_payload && !j->t.pf && !no_fuse)
    {
        // {key, payload} cells: one 16-byte read answers a hit completely (k_join_fuse_payload); rebuilt per call -- the payload column
        // is the caller's, and nothing ties its contents to its address between two calls
        void * fm = nullptr;
        size_t fcls = 0;
        CHGPU_TRY(chgpu_pool_alloc(ctx, (size_t)(cap + 1) * 16, &fm, &fcls));
        hipLaunchKernelGGL(k_join_fuse_payload, dim3(chgpu_grid_for(ctx, cap + 1, JT, 8)), dim3(JT), 0, ctx->stream, j->t, pp, pt, (const u64 *)j->block_base_dev, (u64)j->blocks.size(),
                           (u64 *)fm);
        JoinTable ft = j->t;
        ft.kv = (u64 *)fm;
        probe(k_join_probe_agg_regions<false, true>, ft);
        ctx->counters[6] += 5;
        const hipError_t e = hipGetLastError();
        chgpu_pool_free(ctx, fm, fcls); // reuse is stream-ordered behind the probe
        CHGPU_REQUIRE(e == hipSuccess, CHGPU_ERR_DEVICE, "join probe launch: %s", hipGetErrorString(e));
        return chgpu_read_back(ctx, result2, res, 16);
    }
    probe(j->t.pf ? k_join_probe_agg_regions<true> : k_join_probe_agg_regions<false>, j->t);
    ctx->counters[6] += 4;
    CHGPU_HIP(hipGetLastError());
    return chgpu_read_back(ctx, result2, res, 16);
}

// ---------------------------------------------------------------------------------------------
// LDS-staged probe (unique build keys, integer payload): the probe keys are partitioned TWICE -- 64 contiguous first-level partitions
// by the top bits of the home slot (k_rp_hist_wide + k_rp_scatter, runs of 256 keys), then tile-sorted inside them by the next bits
// (k_rp_tilesort_keys) -- down to table slices of 8192 cells, which one workgroup stages in LDS as {key, payload} (the payload gathered
// through the row id while staging: once per build row, not once per probe row) and then answers every key of that slice from LDS.
// A probe key costs two streaming passes and one LDS look-up instead of an L2 gather; the {key, payload} copy of the table
// (k_join_fuse_payload) is not needed.  A linear-probing chain that runs past the slice end finds the next slice's first JPL2_TAIL cells
// in LDS too, and the global table behind them.
// ---------------------------------------------------------------------------------------------
static constexpr u32 JPL2_LG_CELLS = 12, JPL2_CELLS = 1u << JPL2_LG_CELLS, JPL2_TAIL = 256, JPL2_TILE = jpart_sort_tile(false), JPL2_LG_P1 = 6, JPL2_THREADS = 512;
static_assert(JPL2_LG_CELLS == JBS_LG_CELLS && JPL2_LG_P1 == JBS_LG_P1, "one slice geometry for the slice build and the LDS probe (SliceUnit, join_slice_geom)");
// (4096-cell slices and 512-thread workgroups: two workgroups per CU, so one's staging round trips overlap the other's probing --
//  8192 cells x 1024 threads, one per CU: 0.68 ms for C4's 1e8 keys)

// The radix join has no table whose placement it must match, so it places keys by ONE 64-bit multiply (top lg_cap bits of key x odd
// constant) instead of intHash64's two multiplies and three shift-xors: the hash is evaluated once per key in each of the four passes, and
// a 64-bit multiply is four quarter-rate instructions.  (A key set that clusters under it overflows a slice's window: the stray flag
// sends the call to the table paths.)
__device__ __forceinline__ u64 join_radix_slot(u64 key, u32 lg_cap) { return (key * 0x9E3779B97F4A7C15ull) >> (64 - lg_cap); }
struct JoinRadixFn1
{
    u32 lg_cap, shift;
    __device__ __forceinline__ u32 operator()(u64 key) const { return (u32)(join_radix_slot(key, lg_cap) >> shift); }
};
struct JoinRadixFn2
{
    u32 lg_cap, shift2, lg_p2;
    __device__ __forceinline__ u32 operator()(u64 key, u64 first) const
    {
        const u32 r = (u32)(join_radix_slot(key, lg_cap) >> shift2), r0 = (u32)(join_radix_slot(first, lg_cap) >> shift2) >> lg_p2 << lg_p2;
        return r - r0;
    }
};

// FROM_ROWS: there is no table -- the slice's LDS cells are filled from the BUILD ROWS of the slice, which were partitioned the same way
// (bkeys2 / bwords2 = keys and payloads tile-sorted inside 64 partitions, boff1 / btidx their offsets and run index; t only carries the
// capacity).  A duplicate build key raises dup_flag (the caller then builds the table and takes the other paths).
template <bool FROM_ROWS>
__global__ __launch_bounds__(JPL2_THREADS) void k_join_probe_lds(JoinTable t, int variant, const u64 * __restrict__ keys2, u64 n, const u64 * __restrict__ off1, u32 G, u32 lg_p2,
                                                         const unsigned short * __restrict__ tile_index, const u64 * __restrict__ payload,
                                                         const u64 * __restrict__ block_base, u64 n_blocks, u32 * __restrict__ unit_ctr, u32 * __restrict__ stray_flag,
                                                         unsigned long long * __restrict__ result2, const u64 * __restrict__ bkeys2, const u64 * __restrict__ bwords2,
                                                         const u64 * __restrict__ boff1, const unsigned short * __restrict__ btidx, u64 nb, u32 * __restrict__ dup_flag)
{
    // The hot loop touches global memory only to stream the keys in: everything a key can meet -- its slice, the cells behind it, the
    // zero key's cell -- is staged in LDS first, and the one case that is not (a chain longer than the staged window) raises the
    // stray flag instead of reading the table (the host then discards this run).  A conditional global load inside the loop would
    // make every wait for the prefetched keys a full drain.
    extern __shared__ __attribute__((aligned(16))) unsigned char jpl2_lds[];
    jv2 * cells = (jv2 *)jpl2_lds; // [JPL2_CELLS + JPL2_TAIL] the slice and the cells behind it, then [1] the zero key {present, payload}
    constexpr u32 WIN = JPL2_CELLS + JPL2_TAIL;
    __shared__ u64 s_off[JSL_P1 + 1];
    const u32 PB = 2u << lg_p2;
    __shared__ u64 s_boff[JSL_P1 + 1];
    jpart_stage_offsets(s_off, off1, G, n, JPL2_THREADS);
    if constexpr (FROM_ROWS)
        jpart_stage_offsets(s_boff, boff1, G, nb, JPL2_THREADS);
    const u32 lane = threadIdx.x & 63;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 mask = t.capacity - 1;
    u32 lg_cap = 0;
    while ((1ull << lg_cap) < t.capacity)
        ++lg_cap;
    auto slot_of = [&](u64 key) -> u64 { return FROM_ROWS ? join_radix_slot(key, lg_cap) : (dev_intHash64(key) & mask); };
    if constexpr (!FROM_ROWS)
        if (threadIdx.x == 0)
        {
            const bool hz = t.ctrl->has_zero != 0; // the zero key lives out of line (cell `capacity`)
            cells[WIN] = jv2{hz ? 1ull : 0ull, hz ? payload[join_flat_row(block_base, n_blocks, t.kv[2 * t.capacity + 1])] : 0ull};
            cells[WIN + 1] = jv2{0, 0};
        }
    u64 cnt = 0, isum = 0;
    bool stray = false, dup = false;
    for (;;)
    {
        const u32 r2 = slice_unit_claim(unit_ctr, [] {}); // (its first barrier: the previous unit's cells have been read by everyone)
        if (r2 >= (JSL_P1 << lg_p2))
            break;
        const SliceUnit u = slice_unit(r2, s_off, lg_p2);
        if (u.rb == u.re)
            continue; // no probe key lands in this partition
        // stage the slice, {key, row id} -> {key, payload}: all the cell loads first, then all the payload loads (two round trips, not 2 x 9)
        if constexpr (FROM_ROWS)
        {
            // build the slice's cells from its build rows: LDS compare-and-swap, linear probing inside the window (it is private to this
            // unit, so a chain may run on into the cells behind the slice); the zero key sits in the extra cell
            constexpr u32 NWB = JPL2_THREADS / 64;
            u64 * cw = (u64 *)cells;
            for (u32 c = threadIdx.x; c <= WIN + 1; c += JPL2_THREADS)
                cells[c] = jv2{0, 0};
            __syncthreads();
            const u64 bb = s_boff[u.p1], be = s_boff[u.p1 + 1];
            if (bb != be)
            {
                const u32 bt_lo = (u32)(bb / JBS_TILE), bt_hi = (u32)((be - 1) / JBS_TILE);
                const u32 my_bt = bt_lo + wave <= bt_hi ? (bt_hi - bt_lo - wave) / NWB + 1 : 0;
                auto insert_row = [&](u64 key, u64 pay) {
                    const bool zk = key == 0; // the zero key's cell, behind the window, holds {present, payload}
                    u32 c = zk ? WIN : (u32)(slot_of(key) - u.slice);
                    const int claim = lds_claim<2>(cw, c, zk ? WIN + 1 : WIN, zk ? 1ull : key);
                    if (claim == LDS_CLAIMED)
                        cw[2 * c + 1] = pay; // nobody reads it before the barrier below
                    else if (claim == LDS_DUPLICATE)
                        dup = true;
                    else
                        stray = true; // the window is too short for this chain: not this plan
                };
                // as on the probe side: lane k fetches the run of this wave's k-th build tile, then the rows of TBB tiles are loaded
                // together (a run is ~60 rows: tile by tile the wave sat out an index and a row round trip per tile -- half the kernel)
                for (u32 kb = 0; kb < my_bt; kb += 64)
                {
                    const u32 tile0 = bt_lo + wave + kb * NWB;
                    u32 st_l, ln_l;
                    jpart_lane_runs(s_boff, u, tile0, NWB, my_bt - kb, JBS_TILE, btidx, PB, st_l, ln_l);
                    const u32 nkb = my_bt - kb < 64 ? my_bt - kb : 64;
                    constexpr u32 TBB = 4;
                    for (u32 k0 = 0; k0 < nkb; k0 += TBB)
                    {
                        u64 bkey[TBB], bpay[TBB], brow[TBB];
                        u32 blen[TBB];
#pragma unroll
                        for (u32 q = 0; q < TBB; ++q)
                        {
                            jpart_run_of(st_l, ln_l, k0 + q, nkb, tile0, NWB, JBS_TILE, brow[q], blen[q]);
                            const u64 at = brow[q] + (lane < blen[q] ? lane : 0);
                            bkey[q] = bkeys2[at];
                            bpay[q] = bwords2[at];
                        }
#pragma unroll
                        for (u32 q = 0; q < TBB; ++q)
                        {
                            if (lane < blen[q])
                                insert_row(bkey[q], bpay[q]);
                            for (u32 o = 64 + lane; o < blen[q]; o += 64) // a run longer than a wave (skew)
                                insert_row(bkeys2[brow[q] + o], bwords2[brow[q] + o]);
                        }
                    }
                }
            }
        }
        else
        {
            constexpr u32 NC = (WIN + JPL2_THREADS - 1) / JPL2_THREADS;
            jv2 cl[NC];
#pragma unroll
            for (u32 i = 0; i < NC; ++i)
            {
                const u32 c = threadIdx.x + i * JPL2_THREADS;
                cl[i] = *(const jv2 *)(t.kv + 2 * ((u.slice + (c < WIN ? c : 0)) & mask));
            }
#pragma unroll
            for (u32 i = 0; i < NC; ++i)
                cl[i].y = payload[cl[i].x != 0 ? join_flat_row(block_base, n_blocks, cl[i].y) : 0];
#pragma unroll
            for (u32 i = 0; i < NC; ++i)
            {
                const u32 c = threadIdx.x + i * JPL2_THREADS;
                if (c < WIN)
                    cells[c] = cl[i];
            }
        }
        __syncthreads();
        const u32 t_lo = (u32)(u.rb / JPL2_TILE), t_hi = (u32)((u.re - 1) / JPL2_TILE);
        // This wave's tiles: t_lo + wave, + NW, ...  Lane k fetches the run of tile k (one round trip for all of them instead of one
        // per tile); the keys of tile k + 1 are in flight while tile k is answered from LDS.
        constexpr u32 NW = JPL2_THREADS / 64;
        const u32 my_tiles = t_lo + wave <= t_hi ? (t_hi - t_lo - wave) / NW + 1 : 0;
        // One look-up, straight-line for all but the longest chains: the home cell and its successor are read unconditionally and the
        // answer is selected; the zero key is the same look-up aimed at the extra cell (which holds {1, payload} when present); lanes
        // without a key carry valid = false.  (With a branch per case the loop spent ~100 scalar instructions per 64 look-ups on
        // exec-mask bookkeeping -- PMC: 1.9e8 SALU against 1.4e8 VALU instructions for 1e8 keys -- but removing them did not move the
        // kernel's 0.69 ms: 59 % of its wave cycles are waits)
        auto probe_one = [&](u64 key, bool valid) {
            const bool zk = key == 0;
            const u64 want = zk ? 1ull : key;
            u32 c = zk ? WIN : (u32)(slot_of(key) - u.slice); // the home slot: inside the slice by construction
            const jv2 c0 = cells[c], c1 = cells[c + 1];
            bool found = c0.x == want;
            u64 v = c0.y;
            const bool second = !found && c0.x != 0 && !zk;
            found = found || (second && c1.x == want);
            v = (second && c1.x == want) ? c1.y : v;
            bool more = valid && second && c1.x != want && c1.x != 0; // a chain of three or more cells: rare at this load factor
            if (__any(more))
            {
                if (more)
                {
                    c += 2;
                    jv2 cell = c < WIN ? cells[c] : jv2{0, 0};
                    while (cell.x != want && cell.x != 0 && c + 1 < WIN)
                        cell = cells[++c];
                    stray = stray || (cell.x != want && cell.x != 0); // the chain runs on past the staged window
                    found = cell.x == want;
                    v = cell.y;
                }
            }
            // (the build keys are unique: a hit is one row, whose value word IS the payload)
            u64 add = 0;
            const bool take = pv_account(variant, found, add);
            cnt += valid ? add + (take ? 1 : 0) : 0;
            isum += (valid && take) ? v : 0;
        };
        for (u32 kb = 0; kb < my_tiles; kb += 64)
        {
            const u32 tile0 = t_lo + wave + kb * NW;
            u32 st_l, ln_l;
            jpart_lane_runs(s_off, u, tile0, NW, my_tiles - kb, JPL2_TILE, tile_index, PB, st_l, ln_l);
            const u32 nk = my_tiles - kb < 64 ? my_tiles - kb : 64;
            constexpr u32 U = 2;
            auto load_keys = [&](u64 row, u32 len, u32 o0, u64 (&key)[U]) {
#pragma unroll
                for (u32 u2 = 0; u2 < U; ++u2)
                {
                    const u32 o = o0 + u2 * 64 + lane;
                    key[u2] = __builtin_nontemporal_load(&keys2[row + (o < len ? o : 0)]);
                }
            };
            auto probe_keys = [&](u32 len, u32 o0, const u64 (&key)[U]) {
#pragma unroll
                for (u32 u2 = 0; u2 < U; ++u2)
                    probe_one(key[u2], o0 + u2 * 64 + lane < len);
            };
            // batches of TB tiles: all their key loads are issued before the first look-up (a run is only ~128 keys = two loads per lane:
            // tile by tile, even double-buffered, the wave had two tiles' worth of loads in flight and waited out the latency each time)
            constexpr u32 TB = 8;
            for (u32 k0 = 0; k0 < nk; k0 += TB)
            {
                u64 key[TB][U], row[TB];
                u32 len[TB];
#pragma unroll
                for (u32 q = 0; q < TB; ++q)
                {
                    jpart_run_of(st_l, ln_l, k0 + q, nk, tile0, NW, JPL2_TILE, row[q], len[q]);
                    load_keys(row[q], len[q], 0, key[q]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (u32 q = 0; q < TB; ++q)
                {
                    probe_keys(len[q], 0, key[q]);
                    for (u32 o0 = 64 * U; o0 < len[q]; o0 += 64 * U) // a run longer than 128 keys (skew): the rest, unpipelined
                    {
                        u64 kx[U];
                        load_keys(row[q], len[q], o0, kx);
                        probe_keys(len[q], o0, kx);
                    }
                }
            }
        }
    }
    cnt = wave_reduce_add_u64(cnt);
    isum = wave_reduce_add_u64(isum);
    if (lane == 0 && (cnt || isum))
    {
        atomicAdd(&result2[0], (unsigned long long)cnt);
        atomicAdd(&result2[1], (unsigned long long)isum);
    }
    if (stray)
        *stray_flag = 1;
    if (dup)
        *dup_flag = 1;
}

// -> CHGPU_OK with res[] filled, or NOT_IMPLEMENTED (shape does not fit / a tile straddled three partitions): the caller goes on with the region probe
static int join_probe_agg_lds(chgpu_join * j, const chgpu_col * key_col, const chgpu_col * right_payload, int variant, u64 res[2], u32 * declined)
{
    chgpu_ctx * ctx = j->ctx;
    const u64 n = key_col->rows, cap = j->t.capacity;
    const bool off = chgpu_opt(ctx, "tune_join_no_lds_probe", 0) != 0;
    const u64 min_rows = chgpu_opt(ctx, "tune_join_lds_min_rows", (8ull << 20));
    const JoinSliceGeom geom = join_slice_geom(cap);
    if (off || !j->unique_keys || j->t.pf || !right_payload || chgpu_type_is_float(right_payload->type) || chgpu_type_size(right_payload->type) != 8
        || chgpu_type_size(j->key_type) != 8 || n < min_rows || n + JPL2_TILE + RP_SCATTER_SLACK >= (1ull << 32) || !geom.fits || ((uintptr_t)key_col->data % 16) != 0)
        return CHGPU_ERR_NOT_IMPLEMENTED;
    const u32 lg_cap = geom.lg_cap, lg_p2 = geom.lg_p2, P1 = geom.P1, PB = geom.PB;
    const JoinRegionFn fn1{cap - 1, lg_cap - JPL2_LG_P1};
    const JoinBucket2Fn fn2{cap - 1, JPL2_LG_CELLS, lg_p2};
    const u32 G = (u32)ctx->num_cus;
    u64 * total_dev; // [2..3] the result, [4] unit counter + stray flag
    JoinPart part;
    CHGPU_TRY(join_scratch(ctx, &total_dev, [&](JoinCarve & c) { part = join_part_carve(c, n, G, P1, PB, false); }));
    unsigned long long * result2 = (unsigned long long *)(total_dev + 2);
    u32 * unit_ctr = (u32 *)(total_dev + 4), * stray = unit_ctr + 1;
    CHGPU_TRY(join_partition2<false>(ctx, part, (const u64 *)key_col->data, nullptr, n, P1, fn1, PB, fn2, stray));
    {
        const size_t lds = (size_t)(JPL2_CELLS + JPL2_TAIL + 2) * 16;
        CHGPU_HIP(hipFuncSetAttribute((const void *)k_join_probe_lds<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_join_probe_lds<false>, dim3(2 * G), dim3(JPL2_THREADS), lds, ctx->stream, j->t, variant, (const u64 *)part.keys2, n, (const u64 *)part.offsets, G,
                           lg_p2, (const unsigned short *)part.tidx, (const u64 *)right_payload->data, (const u64 *)j->block_base_dev, (u64)j->blocks.size(), unit_ctr, stray, result2,
                           (const u64 *)nullptr, (const u64 *)nullptr, (const u64 *)nullptr, (const unsigned short *)nullptr, (u64)0, stray);
    }
    ctx->counters[6] += 5;
    CHGPU_HIP(hipGetLastError());
    u64 back[3];
    CHGPU_TRY(chgpu_read_back(ctx, result2, back, 24));
    const u32 stray_v = (u32)(back[2] >> 32);
    *declined = stray_v ? JOIN_DECLINED_STRAY : 0;
    if (stray_v) // the stray flag: some tile spanned three first-level partitions (tiny partitions) or a chain left the window: not this plan
        return CHGPU_ERR_NOT_IMPLEMENTED;
    res[0] = back[0];
    res[1] = back[1];
    return CHGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// The fused probe WITHOUT a hash table in HBM (a radix join): while the table has not been built yet -- the build side is one block of
// staged keys -- both sides are partitioned down to 4096-cell slices of the table that WOULD be built (build rows {key, payload}: 0.16 ms
// for 1e7 rows; probe keys as in join_probe_agg_lds) and k_join_probe_lds<FROM_ROWS> fills every slice's LDS cells from its build
// rows and answers its probe keys.  Neither the global table (0.62 ms to build) nor the per-probe payload gathers exist.  Duplicate
// build keys, an overflowing window or tiny partitions raise a flag: NOT_IMPLEMENTED, and the caller builds the table after all.
// ---------------------------------------------------------------------------------------------
static int join_probe_agg_radix(chgpu_join * j, const chgpu_col * key_col, const chgpu_col * right_payload, int variant, u64 res[2], u32 * declined)
{
    chgpu_ctx * ctx = j->ctx;
    const bool off = chgpu_opt(ctx, "tune_join_no_radix", 0) != 0;
    const u64 min_rows = chgpu_opt(ctx, "tune_join_lds_min_rows", (8ull << 20));
    const u64 n = key_col->rows, nb = j->total_rows;
    if (off || j->finished || j->blocks.size() != 1 || j->blocks[0].valid || nb < (1u << 20) || !right_payload || chgpu_type_is_float(right_payload->type)
        || chgpu_type_size(right_payload->type) != 8 || chgpu_type_size(j->key_type) != 8 || n < min_rows || n + JPL2_TILE + RP_SCATTER_SLACK >= (1ull << 32)
        || nb + JBS_TILE + RP_SCATTER_SLACK >= (1ull << 32) || ((uintptr_t)key_col->data % 16) != 0 || ((uintptr_t)right_payload->data % 16) != 0
        || ((uintptr_t)j->blocks[0].keys % 16) != 0)
        return CHGPU_ERR_NOT_IMPLEMENTED;
    const u64 cap = join_capacity_for(j->ctx, nb);
    const JoinSliceGeom geom = join_slice_geom(cap);
    if (!geom.fits)
        return CHGPU_ERR_NOT_IMPLEMENTED;
    const u32 lg_cap = geom.lg_cap, lg_p2 = geom.lg_p2, P1 = geom.P1, PB = geom.PB;
    const JoinRadixFn1 fn1{lg_cap, lg_cap - JPL2_LG_P1};
    const JoinRadixFn2 fn2{lg_cap, JPL2_LG_CELLS, lg_p2};
    const u32 G = (u32)ctx->num_cus;
    u64 * total_dev; // [2..3] the result, [4] unit counter | stray flag, [5] dup flag
    JoinPart probe, build;
    CHGPU_TRY(join_scratch(ctx, &total_dev, [&](JoinCarve & c) {
        probe = join_part_carve(c, n, G, P1, PB, false);
        build = join_part_carve(c, nb, G, P1, PB, true);
    }));
    unsigned long long * result2 = (unsigned long long *)(total_dev + 2);
    u32 * unit_ctr = (u32 *)(total_dev + 4), * stray = unit_ctr + 1, * dupf = (u32 *)(total_dev + 5);
    // the build side: rows {key, payload}; then the probe side: keys
    CHGPU_TRY(join_partition2<true>(ctx, build, j->blocks[0].keys, (const u64 *)right_payload->data, nb, P1, fn1, PB, fn2, stray));
    CHGPU_TRY(join_partition2<false>(ctx, probe, (const u64 *)key_col->data, nullptr, n, P1, fn1, PB, fn2, stray));
    {
        JoinTable vt{}; // only the capacity is read
        vt.capacity = cap;
        const size_t lds = (size_t)(JPL2_CELLS + JPL2_TAIL + 2) * 16;
        CHGPU_HIP(hipFuncSetAttribute((const void *)k_join_probe_lds<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_join_probe_lds<true>, dim3(2 * G), dim3(JPL2_THREADS), lds, ctx->stream, vt, variant, (const u64 *)probe.keys2, n, (const u64 *)probe.offsets, G,
                           lg_p2, (const unsigned short *)probe.tidx, (const u64 *)nullptr, (const u64 *)nullptr, (u64)1, unit_ctr, stray, result2, (const u64 *)build.keys2,
                           (const u64 *)build.words2, (const u64 *)build.offsets, (const unsigned short *)build.tidx, nb, dupf);
    }
    ctx->counters[6] += 9;
    CHGPU_HIP(hipGetLastError());
    u64 back[4];
    CHGPU_TRY(chgpu_read_back(ctx, result2, back, 32));
    const u32 stray_v = (u32)(back[2] >> 32), dup_v = (u32)back[3];
    *declined = (stray_v ? JOIN_DECLINED_STRAY : 0) | (dup_v ? JOIN_DECLINED_DUP : 0);
    if (stray_v || dup_v) // stray rows / a duplicate build key: not this plan
        return CHGPU_ERR_NOT_IMPLEMENTED;
    res[0] = back[0];
    res[1] = back[1];
    return CHGPU_OK;
}

// The one-pass probe of the global table: every plan above can refuse a shape, this one takes them all
static int join_probe_agg_one_pass(chgpu_join * j, const chgpu_col * key_col, const chgpu_col * null_map, const chgpu_col * right_payload, int variant, u64 res[2])
{
    chgpu_ctx * ctx = j->ctx;
    const u64 n = key_col->rows;
    const bool is_float = right_payload && chgpu_type_is_float(right_payload->type);
    const u32 grid = chgpu_grid_for(ctx, (n + 3) / 4, JT, 8);
    void * scratch = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, ((size_t)grid + 1) * 16, &scratch));
    u64 * partials = (u64 *)scratch;
    u64 * out2 = partials + 2 * (size_t)grid;
    const void * pp = right_payload ? right_payload->data : nullptr;
    const int pt = right_payload ? right_payload->type : CHGPU_U64;
    const u8 * nm = null_map ? (const u8 *)null_map->data : nullptr;
    auto kern = j->t.pf ? (is_float ? k_join_probe_agg<true, true> : k_join_probe_agg<true, false>) : (is_float ? k_join_probe_agg<false, true> : k_join_probe_agg<false, false>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(JT), 0, ctx->stream, j->t, variant, (const void *)key_col->data, j->key_type, nm, n, pp, pt, (const u64 *)j->block_base_dev,
                       (u64)j->blocks.size(), partials);
    auto finish = is_float ? k_join_probe_agg_finish<true> : k_join_probe_agg_finish<false>;
    hipLaunchKernelGGL(finish, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)partials, grid, out2);
    ctx->counters[6] += 2;
    CHGPU_HIP(hipGetLastError());
    return chgpu_read_back(ctx, out2, res, 2 * sizeof(u64));
}

extern "C" int chgpu_join_probe_agg(chgpu_join * j, const chgpu_col * key_col, const chgpu_col * null_map, const chgpu_col * right_payload,
                                    uint64_t * count_out, void * sum_out)
{
    ChgpuDeviceGuard _dev_guard(j ? j->ctx : nullptr);
    CHGPU_REQUIRE(j && key_col && count_out, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(!right_payload || sum_out, CHGPU_ERR_BAD_ARGUMENTS, "sum_out must not be NULL when a payload column is given");
    CHGPU_REQUIRE(key_col->type == j->key_type, CHGPU_ERR_BAD_ARGUMENTS, "left key column has type %d, expected %d", key_col->type, j->key_type);
    if (null_map)
        CHGPU_REQUIRE(null_map->type == CHGPU_U8 && null_map->rows == key_col->rows, CHGPU_ERR_SIZES_MISMATCH, "null map size mismatch");
    CHGPU_REQUIRE(!(j->kind == CHGPU_JOIN_INNER && j->strictness == CHGPU_STRICT_ANY), CHGPU_ERR_NOT_IMPLEMENTED,
                  "INNER ANY consumes right rows across joinBlock calls (setUsedOnce): use chgpu_join_probe");
    CHGPU_REQUIRE(!jf_track_used(j), CHGPU_ERR_NOT_IMPLEMENTED, "RIGHT / FULL joins emit non-joined rows afterwards: use chgpu_join_probe");
    if (right_payload)
    {
        CHGPU_REQUIRE(chgpu_type_size(right_payload->type) != 0, CHGPU_ERR_BAD_ARGUMENTS, "payload type %d", right_payload->type);
        CHGPU_REQUIRE(right_payload->rows == j->total_rows, CHGPU_ERR_SIZES_MISMATCH,
                      "payload column has %llu rows, the right side has %llu (it must be the right blocks' column glued in insertion order)",
                      (unsigned long long)right_payload->rows, (unsigned long long)j->total_rows);
    }
    chgpu_ctx * ctx = j->ctx;
    const u64 n = key_col->rows;
    const int variant = join_probe_variant(j); // (no RIGHT / FULL, no INNER ANY here: ALL_INNER, ALL_LEFT, ANY_LEFT, SEMI_LEFT or ANTI_LEFT)
    u64 res[2] = {0, 0};
    int plan = CHGPU_ERR_NOT_IMPLEMENTED;
    const char * answered = "one_pass";
    u32 declined = 0, regions = 0;
    const bool debug = chgpu_opt(ctx, "debug", 0) != 0;
    j->build_closed = true; // (a probe ends the build phase, as a joinBlock does)
    if (n && !null_map && !j->finished)
    {
        plan = join_probe_agg_radix(j, key_col, right_payload, variant, res, &declined); // no table at all: both sides partitioned, slices built and probed in LDS
        if (plan != CHGPU_OK && plan != CHGPU_ERR_NOT_IMPLEMENTED)
            return plan;
        if (plan == CHGPU_OK)
            answered = "radix";
        else
            join_debug_declined(ctx, "join probe radix", declined);
    }
    if (plan != CHGPU_OK && !j->finished)
        CHGPU_TRY(join_build_table(j));
    if (plan != CHGPU_OK && n && !null_map)
    {
        declined = 0;
        plan = join_probe_agg_lds(j, key_col, right_payload, variant, res, &declined); // table slices staged in LDS (unique keys, integer payload)
        if (plan == CHGPU_OK)
            answered = "lds";
        if (plan == CHGPU_ERR_NOT_IMPLEMENTED)
        {
            join_debug_declined(ctx, "join probe lds", declined);
            plan = join_probe_agg_regions(j, key_col, right_payload, variant, res, &regions); // table regions resident in L2
            if (plan == CHGPU_OK)
                answered = "regions";
            else if (plan == CHGPU_ERR_NOT_IMPLEMENTED)
                join_debug_declined(ctx, "join probe regions", 0);
        }
    }
    if (plan != CHGPU_OK && plan != CHGPU_ERR_NOT_IMPLEMENTED)
        return plan;
    if (n && plan != CHGPU_OK)
        CHGPU_TRY(join_probe_agg_one_pass(j, key_col, null_map, right_payload, variant, res)); // the global table, one pass
    if (debug && n)
        fprintf(stderr, "chgpu: join probe plan=%s rows=%llu build_rows=%llu cap=%llu regions=%u\n", answered, (unsigned long long)n, (unsigned long long)j->total_rows,
                (unsigned long long)join_capacity_for(ctx, j->total_rows), regions);
    *count_out = res[0];
    if (sum_out)
        memcpy(sum_out, &res[1], 8);
    ctx->counters[3] += n;
    ctx->counters[4] += res[0];
    return CHGPU_OK;
}
#include "join_chain.h"
