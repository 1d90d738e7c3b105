// agg_kernels.hip — GROUP BY on the device: Aggregator::executeOnBlock / merge / convertToBlocks for one numeric key
// and POD-state aggregate functions (count, sum, avg).
//
// Reference loops replaced (file:line in the reference checkout):
//   k_agg_rows      Aggregator::executeImplBatch loops A+B (emplaceKey + addBatch)   src/Interpreters/Aggregator.cpp:1010-1206,
//                   HashTable::emplace / findCell                                     src/Common/HashTable/HashTable.h:448-459,901-1027,
//                   IAggregateFunctionHelper::addBatch                                src/AggregateFunctions/IAggregateFunction.h:428-452
//   k_agg_tuples    mergeDataImpl / HashMap::mergeToViaEmplace, resize+reinsert       Aggregator.cpp:2468-2521, HashMap.h:203-233,
//                                                                                     HashTable.h:504-593
//   finalize        convertToBlockImplFinal / insertResultsIntoColumns                Aggregator.cpp:1948-2117
//
// Table geometry mirrors the reference's (HashTable.h:217-330,358-391): power-of-two capacity, linear probing,
// max fill 1/2, growth x4 until 2^23 cells then x2, empty <=> key == 0, the zero key kept out of line (slot index
// == capacity).  Layout is SoA in HBM: keys[capacity+1], then one u64/f64 array per state word, so probes touch only
// 8-byte keys and state updates are single 64-bit atomics.  Placement hash = intHash64 (Hash.h:27-36); CRC32-C is
// only needed where the hash is externally visible (partition_kernels.hip).
//
// Strategies (chgpu_agg_add_block picks by promised / observed cardinality):
//   LDS-STAGED  a per-workgroup open-addressing table in LDS absorbs repeated keys -- the device analogue of the
//               consecutive-key cache, ColumnsHashingImpl.h:313-366 -- and is flushed once per workgroup; k_agg_part_lds in
//               RANGE mode straight over the source columns (k_agg_rows_lds is the older generic form of it);
//   PARTITIONED k_gb_hist -> scan -> k_gb_scatter -> k_gb_units -> k_agg_part_lds, one or two partitioning levels;
//   DIRECT      k_agg_rows_direct, one HBM atomic per row and state word.
// Per-function row masks (the -If combinator, Nullable arguments: chgpu_agg_set_conditions) are tested where a row's
// contribution is made -- add_row for every per-row path, the update loops of the two LDS-staged kernels -- after the row claimed its cell.
// Rows that would push the table over max fill are marked in a pending bitmap; the host grows the table (rehash) and
// re-runs only those rows, which is the reference's resize-on-overflow (HashTable.h:921-944) restructured for a device
// that cannot realloc inside a kernel.
#include "chgpu_internal.h"
#include "radix_partition.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

static constexpr u32 AGG_MAX_AGGS = 8;
static constexpr u32 AGG_MAX_WORDS = 16;
static constexpr u64 AGG_MIN_CAPACITY = 1ull << 22; // 4 Mi cells: >= 2 Mi cells of slack above max fill for the LDS flushes of ~1000 workgroups
static constexpr u32 AGG_LDS_BYTES = 52 * 1024;    // LDS table budget per workgroup (3 workgroups per CU; 2048 cells x 24 B fits)
static constexpr u32 AGG_THREADS = 256;

// The group counter is striped: one same-address atomic per wave and claim serialises at ~10 ns each -- 16 M groups cost
// 160 ms in the counter alone, and a rehash of 16 M cells 2.9 ms instead of 0.2.  A wave adds to (and checks the soft
// limit against) the stripe picked by its workgroup/wave index, each stripe on its own 128-byte line.
static constexpr u32 AGG_STRIPES = 64;
struct AggCtrl
{
    unsigned long long n_groups; // host side only: sum of the stripes, filled in by agg_read_ctrl
    u32 overflow;                // some row hit the max-fill limit and was left pending
    u32 has_zero;
    u32 fatal;                   // table completely full during a flush (cannot happen by construction)
    u32 pad;
    unsigned long long pad2[13];
    unsigned long long stripe[AGG_STRIPES][16]; // occupied cells incl. the zero key, [s][0] is the counter
};
static constexpr size_t AGG_HDR_BYTES = (sizeof(AggCtrl) + 255) / 256 * 256;

// What a function kind needs, one row per CHGPU_AGG_* in the enum's order.  The per-kind update itself stays with add_row / add_vals.
struct AggKind
{
    unsigned char slots;    // argument slots: 0, 1 or 2 (argMin / argMax: arg, then val)
    unsigned char words;    // value words: 1, 2 or 3 (a conditioned function's `seen` word follows them, see agg_layout)
    unsigned char extremum; // it combines by a max or a claim, not by an add: its rows take the DIRECT kernel
    unsigned char result;   // which of its words holds the result (avg: the numerator)
    unsigned char reached;  // which word is non-zero once a row reached it; AGG_SEEN_WORD (== words): none of its own -- the `seen` word behind them, where the layout gave it one
};
static constexpr u32 AGG_N_KINDS = 8;
static constexpr unsigned char AGG_SEEN_WORD = 1; // `reached` of the one-word kinds
static constexpr AggKind AGG_KINDS[AGG_N_KINDS] = {
    {0, 1, 0, 0, AGG_SEEN_WORD}, // count
    {1, 1, 0, 0, AGG_SEEN_WORD}, // sum
    {1, 2, 0, 0, 1},             // avg {numerator, denominator}
    {1, 1, 1, 0, AGG_SEEN_WORD}, // min
    {1, 1, 1, 0, AGG_SEEN_WORD}, // max
    {1, 2, 1, 1, 0}, // any {claim, value}
    {2, 3, 1, 2, 1}, // argMin {val key, claim, arg}
    {2, 3, 1, 2, 1}, // argMax
};
constexpr bool agg_kinds_reached_ok()
{
    for (u32 k = 0; k < AGG_N_KINDS; ++k)
        if (AGG_KINDS[k].reached > AGG_KINDS[k].words || (AGG_KINDS[k].reached == AGG_KINDS[k].words && AGG_KINDS[k].words != AGG_SEEN_WORD))
            return false;
    return true;
}
static_assert(agg_kinds_reached_ok(), "reached names one of the kind's own words, or -- for a one-word kind only -- the seen word behind it");
static_assert(CHGPU_AGG_COUNT == 0 && CHGPU_AGG_SUM == 1 && CHGPU_AGG_AVG == 2 && CHGPU_AGG_MIN == 3 && CHGPU_AGG_MAX == 4 && CHGPU_AGG_ANY == 5 &&
                  CHGPU_AGG_ARG_MIN == 6 && CHGPU_AGG_ARG_MAX == 7,
              "AGG_KINDS is indexed by CHGPU_AGG_*");
static constexpr bool agg_kind_known(int kind) { return kind >= 0 && (u32)kind < AGG_N_KINDS; }
static constexpr const AggKind & agg_kind(int kind) { return AGG_KINDS[kind]; }

// What each state word of an aggregation is: one bit per word and class.  The aggregator holds one, a kernel's descriptor embeds one
// (a pass over some of the functions: re-expressed in its local numbering, agg_localise_words), the merge kernels take one as it is.
struct AggWords
{
    u32 n_words;     // every word, the appended high halves of the fixed-point sums included
    u32 n_pub_words; // the first n_pub_words are the words the C ABI shows (state columns, wire format)
    u32 f64;         // bit w: word w combines by a Float64 add
    u32 max;         // bit w: word w combines by an unsigned max (min / max order keys, any()'s claim), never by an add
    // deterministic Float64 sums (see Fx128): bit w of fx = word w is the LOW half of a 128-bit fixed-point sum whose high half is word
    // fx_hi[w] (one of the words appended behind the regular ones, bit fx_hi[w] of fx_high: never updated on its own)
    u32 fx, fx_high;
    u32 any;  // bit w: word w is any()'s claim, word w + 1 its value
    u32 arg;  // bit w: words w, w + 1, w + 2 are the {val key, claim, arg} of an argMin / argMax
    u32 seen; // bit w: word w counts the rows that reached the conditioned function whose value word(s) end at w - 1
    unsigned char fx_hi[AGG_MAX_WORDS];
    // how word w combines, as global_add_word takes it: 0 integer add, 1 Float64 add, 2 unsigned max
    __host__ __device__ __forceinline__ int op(u32 w) const { return ((max >> w) & 1) ? 2 : (int)((f64 >> w) & 1); }
    // the type of public word w's state column (a fixed-point pair leaves as the Float64 it stands for)
    int pub_type(u32 w) const { return (((f64 | fx) >> w) & 1) ? CHGPU_F64 : CHGPU_U64; }
};

// An AggWords as k_agg_tuples takes it.  That kernel uses the last SGPR that still gives 8 waves per SIMD and every mask is live across
// its row loop, so the two combine masks travel in one word there: bit w of `ops` = Float64 add, bit AGG_MAX_WORDS + w = unsigned max.
// The members a merge never reads stay behind.  Same member names and op(w) as AggWords: ovf_flush takes either.
struct AggMergeWords
{
    u32 n_words, ops, fx, fx_high, any, arg;
    unsigned char fx_hi[AGG_MAX_WORDS];
    explicit AggMergeWords(const AggWords & ws)
        : n_words(ws.n_words), ops(ws.f64 | (ws.max << AGG_MAX_WORDS)), fx(ws.fx), fx_high(ws.fx_high), any(ws.any), arg(ws.arg)
    {
        memcpy(fx_hi, ws.fx_hi, sizeof(fx_hi));
    }
    __device__ __forceinline__ int op(u32 w) const { return ((ops >> (AGG_MAX_WORDS + w)) & 1) ? 2 : (int)((ops >> w) & 1); }
};
static_assert(2 * AGG_MAX_WORDS <= 32, "AggMergeWords::ops holds two masks");

struct AggArg
{
    const void * ptr; // argument column (NULL for count); argMin / argMax: the `arg` column, the one the result comes from
    const void * val; // argMin / argMax: the `val` column, the one that is compared
    int kind;
    int arg_type;
    int val_type;
    u32 word;         // first state word
    u32 pre;          // partitioned path: index of this argument's word column in the partition buffers
    // -If / -Null combinators: the function sees row i only when (AggDesc::cond[cond][i] != 0) == cond_want
    signed char cond;       // index into AggDesc::cond, -1 = unconditioned
    unsigned char cond_want; // 1: -If (the byte is non-zero), 0: Nullable argument (the null-map byte is zero)
    unsigned char seen;      // 1: word + 1 counts the rows that reached the function (conditioned min / max, NULL-mode sum)
};

struct AggDesc
{
    // The ORDER of the members is chosen by what the compiler makes of it: the struct is a kernel argument, and the SGPR spills of the
    // LDS-staged kernels follow its layout (profiles/agg_state_words_resources.md).  Reorder only with the resource table at hand.
    // A pass over a SUBSET of the functions (one argument word at a time through the tile-sorted plan) numbers its state words locally
    // (0 .. n_words - 1: the LDS cells hold only those) and finds the table's words through this map; the identity otherwise.
    unsigned char word_map[AGG_MAX_WORDS];
    // argMin / argMax: the claim a raised extremum falls back to, that of the ordinal behind the block's last row: below the claim of
    // every row of this and every earlier block (see raise_extremum)
    u64 arg_sentinel;
    u32 n_aggs;
    int fx_base; // the fixed-point sums' values are multiples of 2^fx_base
    u64 row_seq; // any(): row i of the argument columns is the (row_seq + i)-th row this aggregation has seen (modulo 2^64)
    // (`arg` and `any` are in table numbering: such rows take the DIRECT kernel, which numbers nothing locally; the localised form of a
    // subset pass -- additive functions only -- has neither, nor `seen`)
    AggWords words;
    // the distinct condition columns of the block (UInt8, indexed like the arguments); n_conds = 0: no function is conditioned
    const u8 * cond[AGG_MAX_AGGS];
    u32 n_conds;
    AggArg a[AGG_MAX_AGGS];
};

struct AggTable
{
    u64 * keys;      // [capacity + 1]
    u64 * words;     // [n_words][capacity + 1]
    u64 capacity;    // power of two
    u64 max_fill;    // capacity / 2
    AggCtrl * ctrl;
    // find-only mode (no_more_keys): keys are looked up, never inserted; the state of a key the table lacks goes to the overflow row
    // `ovf` ([n_words] words, the layout of one cell) or is dropped when ovf is NULL.  0 for ordinary blocks and for the rehash.
    u32 find_only = 0;
    u64 * ovf = nullptr;
};

struct chgpu_agg
{
    chgpu_ctx * ctx = nullptr;
    int key_type = -1;
    u32 n_aggs = 0;
    int kinds[AGG_MAX_AGGS];
    int arg_types[AGG_MAX_AGGS];
    int val_types[AGG_MAX_AGGS]; // argMin / argMax: the type of `val` (arg_types[j] is `arg`'s, the result's)
    u32 slot[AGG_MAX_AGGS];      // the aggregate's first argument slot: arg_cols[] is indexed by slot, argMin / argMax own two (arg, val)
    u32 n_slots = 0;
    u32 word_off[AGG_MAX_AGGS];
    // The state words (agg_layout).  any(): claim = ~(ordinal of the row that set the value) under an unsigned max: the EARLIEST row of
    // the group wins whatever order the hardware serves the rows in; the value is stored by a second pass from the winner's row
    // (k_agg_any_resolve).  argMin / argMax: the val key combines like a min / max word, the claim names the earliest row (or merged
    // state) that holds that extremum, the arg is stored from the claim's row (k_agg_arg_rows).
    AggWords words{};
    u64 size_hint = 0;
    AggTable t{nullptr, nullptr, 0, 0, nullptr};
    void * table_mem = nullptr; // from the context's column pool (stream-ordered reuse: no hipMalloc/hipFree per query)
    size_t table_class = 0;
    u64 n_groups = 0; // host copy, refreshed after every call
    bool hint_probed = false; // the cardinality of a hint-less aggregation was sampled on its first large block
    bool has_extremum = false; // some function is min / max / any: rows take the DIRECT kernel (the LDS-staged plans only know how to add)
    u64 any_seq = 0;  // rows seen so far
    u64 nokey_kept = 0; // without key: rows that reached the states (0 = min / max / any have no value: insertResultInto gives the default)
    // deterministic Float64 sums (option deterministic_float_sums, the default): sum / avg over a float argument keep a 128-bit fixed-point
    // state {word, words.fx_hi[word]} in units of 2^fx_base instead of a double; exports fold a pair back into its Float64 column.
    // window invariant: every state is a sum of at most fx_rows values, each below 2^(127 - fx_log_cap) units of 2^fx_base
    int fx_base = 0;
    bool fx_base_set = false;
    u64 fx_rows = 0;
    int fx_log_cap = 30;
    int fx_emin = 4096; // smallest (unbiased) exponent among the non-zero values added so far
    u64 host_words[AGG_MAX_WORDS]; // without_key states live on the host (8 B each)
    // max_rows_to_group_by / group_by_overflow_mode / overflow_row (Aggregator::Params); set before the first block
    u64 max_rows = 0;
    int overflow_mode = CHGPU_OVERFLOW_THROW;
    bool overflow_row = false;
    bool started = false;          // some block or merge has reached the aggregation
    void * ovf_mem = nullptr;      // the overflow row's state words on the device (AGG_MAX_WORDS x 8 B), from the first call with overflow_row on
    size_t ovf_class = 0;
    // -If / -Null combinators (chgpu_agg_set_conditions): CHGPU_AGG_COND_* per function
    int cond_modes[AGG_MAX_AGGS] = {0};
    bool conditioned = false;
    const chgpu_col * const * block_conds = nullptr; // the condition columns of the block being added ([n_aggs], set for the call's duration)
};

// ---------------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 load_key_zext(const void * keys, int type, u64 i)
{
    // HashMethodOneNumber::getKeyHolder (ColumnsHashing/HashMethod.h:91): raw bits of the key, zero-extended to the
    // UInt64 table key (AggregatedDataVariants.h:63-64)
    switch (type)
    {
        case CHGPU_U32: case CHGPU_I32: return ((const u32 *)keys)[i];
        case CHGPU_U16: case CHGPU_I16: return ((const u16 *)keys)[i];
        case CHGPU_U8: case CHGPU_I8: return ((const u8 *)keys)[i];
        default: return ((const u64 *)keys)[i];
    }
}

__device__ __forceinline__ u64 load_arg_bits(const void * p, int type, u64 i)
{
    switch (type)
    {
        case CHGPU_I64: case CHGPU_U64: case CHGPU_F64: return ((const u64 *)p)[i];
        case CHGPU_U32: return ((const u32 *)p)[i];
        case CHGPU_I32: return (u64)(i64)((const i32 *)p)[i]; // sign-extend: wrap-around two's complement sum
        case CHGPU_U8: return ((const u8 *)p)[i];
        case CHGPU_U16: return ((const u16 *)p)[i];
        case CHGPU_I16: return (u64)(i64)((const i16 *)p)[i];
        case CHGPU_I8: return (u64)(i64)((const i8 *)p)[i];
        case CHGPU_F32: return (u64)__double_as_longlong((double)((const float *)p)[i]); // Float32 is accumulated as Float64
        default: return 0;
    }
}

// op: 0 = wrap-around integer add, 1 = Float64 add, 2 = unsigned max (min / max states: order keys, see agg_order_key)
__device__ __forceinline__ void global_add_word(u64 * p, u64 bits, int op)
{
    if (op == 2)
    {
        if (bits) // (0 is the identity: nothing to do)
            __hip_atomic_fetch_max((unsigned long long *)p, (unsigned long long)bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const bool is_f64 = op == 1;
    if (is_f64)
        __hip_atomic_fetch_add((double *)p, __longlong_as_double((long long)bits), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        __hip_atomic_fetch_add((unsigned long long *)p, (unsigned long long)bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- deterministic Float64 sums -------------------------------------------------------------------------------------------------
// A double atomicAdd makes a group's sum depend on the order the hardware happened to serve the rows in (the reference is deterministic
// for a fixed block split: AggregateFunctionSum.h:72-101 adds in row order).  Integer addition is associative, so the state of sum /
// avg over a float argument is a two's complement 128-bit integer in units of 2^base instead: every row contributes trunc(x * 2^-base),
// whatever the order, the plan or the number of workgroups.  base = (largest exponent seen) - 96: the window holds 2^30 rows of the
// largest magnitude and keeps every bit of values down to 2^-44 of it (2^-20 relative precision down to 2^-76 of it) -- the host widens
// the window (an arithmetic shift of every state) when a block brings a larger exponent or the row count outgrows the head room.
// The two halves are separate words: low += x.lo returns the old value, and the adder that sees the wrap carries into the high word --
// each wrap is seen by exactly one adder, so the pair ends at the exact sum.
struct Fx128
{
    u64 lo, hi;
};
__device__ __host__ __forceinline__ Fx128 fx_from_double(u64 bits, int base)
{
    const u32 e = (u32)(bits >> 52) & 0x7ffu;
    u64 m = bits & 0xFFFFFFFFFFFFFull;
    if (e)
        m |= 1ull << 52;
    const int sh = (int)(e ? e : 1u) - 1075 - base; // x = m * 2^(e - 1075)
    Fx128 r;
    if (sh >= 64)
        r.lo = 0, r.hi = sh < 128 ? m << (sh - 64) : 0; // (sh + 53 <= 97 by the choice of base)
    else if (sh > 0)
        r.lo = m << sh, r.hi = m >> (64 - sh);
    else if (sh > -64)
        r.lo = m >> -sh, r.hi = 0;
    else
        r.lo = 0, r.hi = 0;
    if (bits >> 63)
    {
        r.lo = ~r.lo + 1;
        r.hi = ~r.hi + (r.lo == 0 ? 1 : 0);
    }
    return r;
}
// the pair as the nearest double (ties to even): the only rounding of the whole sum
__device__ __host__ __forceinline__ double fx_to_double(u64 lo, u64 hi, int base)
{
    const bool neg = (hi >> 63) != 0;
    if (neg)
    {
        lo = ~lo + 1;
        hi = ~hi + (lo == 0 ? 1 : 0);
    }
    if ((lo | hi) == 0)
        return 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
    const int top = hi ? 127 - __clzll((long long)hi) : 63 - __clzll((long long)lo);
#else
    const int top = hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);
#endif
    u64 m;
    int sh = top - 52; // bits dropped
    if (sh <= 0)
        m = lo, sh = 0; // (top <= 52: the magnitude is exact in a double)
    else
    {
        // m = magnitude >> sh, rem = the dropped bits against one half
        u64 rem_hi, rem_lo; // dropped bits, left-aligned in 128 bits
        if (sh < 64)
        {
            m = (lo >> sh) | (hi << (64 - sh));
            rem_hi = lo << (64 - sh);
            rem_lo = 0;
        }
        else if (sh == 64)
        {
            m = hi;
            rem_hi = lo;
            rem_lo = 0;
        }
        else
        {
            m = hi >> (sh - 64);
            rem_hi = (hi << (128 - sh)) | (lo >> (sh - 64));
            rem_lo = lo << (128 - sh);
        }
        const u64 half = 1ull << 63;
        if (rem_hi > half || (rem_hi == half && (rem_lo != 0 || (m & 1))))
            ++m; // (2^53 is a double too)
    }
    const double v = ldexp((double)m, sh + base);
    return neg ? -v : v;
}
__device__ __forceinline__ void global_add_fx(u64 * lo, u64 * hi, Fx128 x)
{
    u64 h = x.hi;
    if (x.lo)
    {
        const u64 old = __hip_atomic_fetch_add((unsigned long long *)lo, (unsigned long long)x.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        h += (old + x.lo < old) ? 1 : 0;
    }
    if (h)
        __hip_atomic_fetch_add((unsigned long long *)hi, (unsigned long long)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lds_add_fx(u64 * lo, u64 * hi, Fx128 x)
{
    u64 h = x.hi;
    if (x.lo)
    {
        const u64 old = atomicAdd((unsigned long long *)lo, (unsigned long long)x.lo);
        h += (old + x.lo < old) ? 1 : 0;
    }
    if (h)
        atomicAdd((unsigned long long *)hi, (unsigned long long)h);
}

// Find-or-claim the cell of `key` (emplace).  Returns the slot, or ~0 when the row must wait for a bigger table.
// soft_limit: refuse to claim new cells once n_groups >= max_fill (rows); flushes/rehash pass false and may use
// the slack above max fill.  Every loop is bounded by the capacity, so the wave always exits.
__device__ __forceinline__ u32 agg_stripe() { return (blockIdx.x * 5 + (threadIdx.x >> 6)) & (AGG_STRIPES - 1); }

__device__ __forceinline__ void count_claim(const AggTable & t, bool claimed)
{
    // one atomic per wave, on the wave's stripe of the group counter
    const u64 cb = __ballot(claimed);
    if (claimed && mbcnt(cb) == 0)
        atomicAdd(&t.ctrl->stripe[agg_stripe()][0], (unsigned long long)__popcll(cb));
}
__device__ __forceinline__ u64 table_emplace_impl(const AggTable & t, u64 key, bool soft_limit, bool & claimed)
{
    claimed = false;
    if (key == 0)
    {
        // zero key lives out of line (HashTable.h:874-898)
        if (__hip_atomic_load(&t.ctrl->has_zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
            if (atomicExch(&t.ctrl->has_zero, 1u) == 0)
                claimed = true;
        return t.capacity;
    }
    const u64 mask = t.capacity - 1;
    u64 slot = dev_intHash64(key) & mask;
    for (u64 step = 0; step < t.capacity; ++step)
    {
        u64 k = t.keys[slot];
        if (k == key)
            return slot;
        if (k == 0)
        {
            if (soft_limit && __hip_atomic_load(&t.ctrl->stripe[agg_stripe()][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= t.max_fill / AGG_STRIPES)
                return ~0ull;
            const u64 prev = atomicCAS((unsigned long long *)&t.keys[slot], 0ull, (unsigned long long)key);
            if (prev == 0)
            {
                claimed = true;
                return slot;
            }
            if (prev == key)
                return slot;
        }
        slot = (slot + 1) & mask;
    }
    return ~0ull;
}

__device__ __forceinline__ u64 table_emplace(const AggTable & t, u64 key, bool soft_limit)
{
    bool claimed;
    const u64 slot = table_emplace_impl(t, key, soft_limit, claimed);
    count_claim(t, claimed);
    return slot;
}

// min / max states (AggregateFunctionsMinMax.cpp, SingleValueDataFixed<T>::setIfSmaller / setIfGreater, SingleValueData.cpp:219-262): the
// state word holds an ORDER KEY -- the value mapped to an unsigned 64-bit integer that sorts like the value (unsigned: itself; signed: sign
// bit flipped; floats: the IEEE total-order fold, Float32 after its exact widening) -- for max, and its complement for min, combined with
// an unsigned atomic max.  A freshly zeroed cell is then the identity of both, exactly like the sums' zero: the rehash, the merges and the
// exports move min / max words with no special case but the combining operation.  (A group only exists because a row created it, so
// `has()` is always true for it.  Under a per-function condition that no longer holds: a conditioned min / max carries a `seen` word, the
// number of rows that reached it, and finalize gives the type's default when it is 0 -- DESIGN.md §4.16.2.)  NaNs take their total-order place -- above +inf / below -inf by sign -- where the reference's answer
// depends on which row came first (`NaN < x` is false either way).  agg_order_key / agg_order_key_inverse themselves are in
// chgpu_internal.h: the window operator's running min / max (window_kernels.hip) orders by the same key.

// argMin / argMax compare `val` with the reference's operator > / <, to which the two zeros are equal: the val key folds the zero's
// sign away (val is never returned, so nothing is lost).  min / max keep agg_order_key: they return the value.
__device__ __host__ __forceinline__ u64 agg_val_key(u64 bits, int type)
{
    if ((type == CHGPU_F64 || type == CHGPU_F32) && (bits << 1) == 0)
        bits = 0;
    return agg_order_key(bits, type);
}
// argMin / argMax claims.  A row's claim is ~(ordinal + 1): as any()'s, but below ~0, which is kept for "older than every row".  A
// state that arrives by a merge claims with AGG_MERGE_CLAIM_TOP - its index among the source tuples: below every row's claim (ordinals
// stay under 2^63), so a destination that holds the same extremum keeps its own, above AGG_MERGE_SENTINEL, and the earliest source wins
// among several.  The winner then sets the claim to ~0: older than every row to come.
static constexpr u64 AGG_MERGE_CLAIM_TOP = 0x7FFFFFFFFFFFFFFFull;
static constexpr u64 AGG_MERGE_SENTINEL = 1;
__device__ __host__ __forceinline__ u64 agg_arg_row_claim(u64 ordinal) { return ~ordinal - 1; }
// The first pass of an argMin / argMax update: raise the val key; whoever raised it also pulls the claim down to `sentinel`, because the
// claim then names a row that holds the OLD extremum.  The rows (states) that hold the final extremum claim after the kernel boundary.
__device__ __forceinline__ void raise_extremum(u64 * val, u64 * claim, u64 key, u64 sentinel)
{
    if (key == 0)
        return; // the identity
    const u64 old = __hip_atomic_fetch_max((unsigned long long *)val, (unsigned long long)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (key > old)
        __hip_atomic_fetch_min((unsigned long long *)claim, (unsigned long long)sentinel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Where a group's state lives.  A sink has three members: at(w) = the address of TABLE word w, add_word(p, bits, op) (op as in
// global_add_word) and add_fx(lo, hi, x).  GlobalSink is a cell of the HBM table; LdsRowSink (below, with the overflow row) is a
// workgroup's LDS copy of the overflow row.
struct GlobalSink
{
    u64 * words;
    u64 stride, slot;
    __device__ __forceinline__ GlobalSink(const AggTable & t, u64 slot_) : words(t.words), stride(t.capacity + 1), slot(slot_) {}
    __device__ __forceinline__ u64 * at(u32 w) const { return words + (u64)w * stride + slot; }
    __device__ __forceinline__ void add_word(u64 * p, u64 bits, int op) const { global_add_word(p, bits, op); }
    __device__ __forceinline__ void add_fx(u64 * lo, u64 * hi, Fx128 x) const { global_add_fx(lo, hi, x); }
    __device__ __forceinline__ void raise(u64 * val, u64 * claim, u64 key, u64 sentinel) const { raise_extremum(val, claim, key, sentinel); }
};

// add row i's contribution of every aggregate to the group's state in `sink` (IAggregateFunction::add per function)
// Which condition columns hold a non-zero byte in row i (bit c: AggDesc::cond[c]): every distinct column is loaded once per row,
// however many functions share it.  (Any non-zero byte counts: 2 and 255 as much as 1.)
__device__ __forceinline__ u32 cond_row_bits(const AggDesc & d, u64 i)
{
    u32 nz = 0;
    for (u32 c = 0; c < d.n_conds; ++c)
        nz |= (u32)(__builtin_nontemporal_load(d.cond[c] + i) != 0) << c;
    return nz;
}
// does row i (its condition bits `nz`) reach the function?
__device__ __forceinline__ bool cond_reaches(const AggArg & a, u32 nz) { return a.cond < 0 || ((nz >> a.cond) & 1u) == a.cond_want; }

template <typename Sink>
__device__ __forceinline__ void add_row(const Sink & sink, const AggDesc & d, u64 i)
{
    const u32 nz = cond_row_bits(d, i);
    for (u32 j = 0; j < d.n_aggs; ++j)
    {
        const AggArg & a = d.a[j];
        if (!cond_reaches(a, nz))
            continue; // (the cell is claimed all the same: the group exists, AggregateFunctionIf::add / AggregateFunctionNullUnary::add skip)
        u64 * w = sink.at(d.word_map[a.word]);
        if (a.seen)
            sink.add_word(sink.at(d.word_map[a.word] + 1), 1, 0);
        if (a.kind == CHGPU_AGG_COUNT)
            sink.add_word(w, 1, 0);
        else if (a.kind == CHGPU_AGG_MIN || a.kind == CHGPU_AGG_MAX)
        {
            const u64 k = agg_order_key(load_arg_bits(a.ptr, a.arg_type, i), a.arg_type);
            sink.add_word(w, a.kind == CHGPU_AGG_MAX ? k : ~k, 2);
        }
        else if (a.kind == CHGPU_AGG_ANY)
            sink.add_word(w, ~(d.row_seq + i), 2); // the claim of the earliest row; its value follows in k_agg_any_resolve
        else if (a.kind == CHGPU_AGG_ARG_MIN || a.kind == CHGPU_AGG_ARG_MAX)
        {
            const u64 k = agg_val_key(load_arg_bits(a.val, a.val_type, i), a.val_type);
            sink.raise(w, sink.at(d.word_map[a.word] + 1), a.kind == CHGPU_AGG_ARG_MAX ? k : ~k, d.arg_sentinel); // claim and arg: k_agg_arg_rows
        }
        else
        {
            if ((d.words.fx >> a.word) & 1)
                sink.add_fx(w, sink.at(d.word_map[d.words.fx_hi[a.word]]), fx_from_double(load_arg_bits(a.ptr, a.arg_type, i), d.fx_base));
            else
                sink.add_word(w, load_arg_bits(a.ptr, a.arg_type, i), a.arg_type == CHGPU_F64 || a.arg_type == CHGPU_F32);
            if (a.kind == CHGPU_AGG_AVG)
                sink.add_word(sink.at(d.word_map[a.word] + 1), 1, 0); // denominator
        }
    }
}

// The same update from values already in registers: `bits0/bits1` are the 8-byte argument words selected by AggArg::pre,
// `cnt` the number of rows they stand for.
template <typename Sink>
__device__ __forceinline__ void add_vals(const Sink & sink, const AggDesc & d, u64 bits0, u64 bits1, u64 cnt)
{
    for (u32 j = 0; j < d.n_aggs; ++j)
    {
        const AggArg & a = d.a[j];
        u64 * w = sink.at(d.word_map[a.word]);
        if (a.kind == CHGPU_AGG_COUNT)
            sink.add_word(w, cnt, 0);
        else
        {
            if ((d.words.fx >> a.word) & 1)
                sink.add_fx(w, sink.at(d.word_map[d.words.fx_hi[a.word]]), fx_from_double(a.pre == 0 ? bits0 : bits1, d.fx_base));
            else
                sink.add_word(w, a.pre == 0 ? bits0 : bits1, a.arg_type == CHGPU_F64 || a.arg_type == CHGPU_F32);
            if (a.kind == CHGPU_AGG_AVG || a.seen)
                sink.add_word(sink.at(d.word_map[a.word] + 1), cnt, 0); // denominator; the `seen` word of a NULL-mode sum
        }
    }
}

// ---- find-only mode and the overflow row (Aggregator::executeImplBatch with no_more_keys, Aggregator.cpp:1181-1194) ----
// In find-only mode only the step where a group's state leaves the workgroup changes -- the flush of an LDS cell, a row's global update:
// it calls table_find instead of table_emplace, and a miss (AGG_SLOT_MISS) goes to the overflow row.  A workgroup combines its misses in
// an LDS copy of the overflow row (LdsRowSink: LDS atomics) and issues at most one global update per state word at its end (ovf_flush):
// per-row atomics on one global address would serialise.
static constexpr u64 AGG_SLOT_MISS = ~1ull;
__device__ __forceinline__ u64 table_find(const AggTable & t, u64 key)
{
    if (key == 0)
        return __hip_atomic_load(&t.ctrl->has_zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? t.capacity : AGG_SLOT_MISS;
    const u64 mask = t.capacity - 1;
    u64 slot = dev_intHash64(key) & mask;
    for (u64 step = 0; step < t.capacity; ++step)
    {
        const u64 k = t.keys[slot];
        if (k == key)
            return slot;
        if (k == 0)
            return AGG_SLOT_MISS;
        slot = (slot + 1) & mask;
    }
    return AGG_SLOT_MISS;
}
// emplace, or find in find-only mode (t.find_only is uniform over the launch)
__device__ __forceinline__ u64 table_place(const AggTable & t, u64 key, bool soft_limit)
{
    return t.find_only ? table_find(t, key) : table_emplace(t, key, soft_limit);
}
__device__ __forceinline__ void ovf_lds_init(u64 * s)
{
    if (threadIdx.x < AGG_MAX_WORDS)
        s[threadIdx.x] = 0;
}
// op: 0 integer add, 1 Float64 add, 2 unsigned max (as global_add_word)
__device__ __forceinline__ void ovf_lds_word(u64 * s, u64 bits, int op)
{
    if (op == 2)
    {
        if (bits)
            atomicMax((unsigned long long *)s, (unsigned long long)bits);
    }
    else if (op == 1)
        atomicAdd((double *)s, __longlong_as_double((long long)bits));
    else if (bits)
        atomicAdd((unsigned long long *)s, (unsigned long long)bits);
}
// the LDS copy s[] of the overflow row as a sink, indexed by table word.  One deliberate difference from GlobalSink: an integer add
// of zero is skipped here (ovf_lds_word) and issued there.
struct LdsRowSink
{
    u64 * s;
    __device__ __forceinline__ u64 * at(u32 w) const { return s + w; }
    __device__ __forceinline__ void add_word(u64 * p, u64 bits, int op) const { ovf_lds_word(p, bits, op); }
    __device__ __forceinline__ void add_fx(u64 * lo, u64 * hi, Fx128 x) const { lds_add_fx(lo, hi, x); }
    // argMin / argMax: the workgroup's largest val key; ovf_flush raises the overflow row's with it (the LDS claim word stays unused)
    __device__ __forceinline__ void raise(u64 * val, u64 *, u64 key, u64) const { ovf_lds_word(val, key, 2); }
};
// local state word w of a flushed LDS cell (bits; hb = its fixed-point high half), to the group's state in `sink`
template <typename Sink>
__device__ __forceinline__ void add_cell_word(const Sink & sink, const AggDesc & d, u32 w, u64 bits, u64 hb)
{
    if ((d.words.fx >> w) & 1)
    {
        if (bits | hb)
            sink.add_fx(sink.at(d.word_map[w]), sink.at(d.word_map[d.words.fx_hi[w]]), Fx128{bits, hb});
    }
    else if (bits != 0)
        sink.add_word(sink.at(d.word_map[w]), bits, (d.words.f64 >> w) & 1); // (an LDS cell holds additive words only: no max to test)
}
// Place a row or leave it pending: `add(sink)` adds the row's contribution to the cell of `key`, or, in find-only mode, to the overflow
// row `s_ovf` (when there is one) if the table lacks the key.  Returns true when the row must wait for a bigger table.
template <typename Add>
__device__ __forceinline__ bool place_and_add(const AggTable & t, u64 * s_ovf, u64 key, bool soft_limit, Add add)
{
    const u64 slot = table_place(t, key, soft_limit);
    if (slot == ~0ull)
        return true;
    if (slot == AGG_SLOT_MISS)
    {
        if (t.ovf)
            add(LdsRowSink{s_ovf});
    }
    else
        add(GlobalSink(t, slot));
    return false;
}
// The workgroup's combined misses to the overflow row: one global update per state word (call after a barrier, every thread).  Local
// words 0 .. n_words-1 of `ws` map to table words through `map` (NULL: the identity).
// merge: any() {claim, value} pairs arrive together (the first state that claims the overflow row keeps it, changeFirstTime) -- a
// row's claim instead combines by max and its value is stored by the winning row later (k_agg_any_resolve).
// ws.arg: argMin / argMax val keys (table words): raised like a cell's, with `arg_sentinel`; their claim and arg words follow in the
// claim and resolve passes.
template <typename Words> // AggWords or AggMergeWords
__device__ __forceinline__ void ovf_flush(const AggTable & t, const u64 * s, const Words & ws, const unsigned char * map, bool merge, u64 arg_sentinel)
{
    const u32 w = threadIdx.x;
    const u32 any_merge = merge ? ws.any : 0;
    if (!t.ovf || w >= ws.n_words || ((ws.fx_high >> w) & 1) || (w > 0 && ((any_merge >> (w - 1)) & 1)))
        return;
    const u32 gw = map ? map[w] : w;
    if ((((ws.arg << 1) | (ws.arg << 2)) >> gw) & 1)
        return; // a claim or an arg word
    const u64 bits = s[gw];
    if ((ws.arg >> gw) & 1)
    {
        raise_extremum(t.ovf + gw, t.ovf + gw + 1, bits, arg_sentinel);
        return;
    }
    if ((any_merge >> w) & 1)
    {
        if (bits && atomicCAS((unsigned long long *)(t.ovf + gw), 0ull, (unsigned long long)bits) == 0ull)
            __hip_atomic_store((unsigned long long *)(t.ovf + gw + 1), (unsigned long long)s[gw + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if ((ws.fx >> w) & 1)
    {
        const u32 gh = map ? map[ws.fx_hi[w]] : ws.fx_hi[w];
        if (bits | s[gh])
            global_add_fx(t.ovf + gw, t.ovf + gh, Fx128{bits, s[gh]});
        return;
    }
    if (bits != 0)
        global_add_word(t.ovf + gw, bits, ws.op(w));
}
__device__ __forceinline__ void ovf_flush_desc(const AggTable & t, const u64 * s, const AggDesc & d)
{
    ovf_flush(t, s, d.words, d.word_map, false, d.arg_sentinel);
}

// ---- the workgroup's LDS table of the LDS-staged kernels ----
// Layout: keys KT[S+1] (padded to 8 B) | every 8-byte word u64[S+1] in word order | every 4-byte word u32[S+1]; cell S is the zero
// key's.  Bit w of cnt32: state word w is a row COUNT kept as 32 bits (see k_agg_part_lds).
struct PartLds
{
    u32 S1, cnt32, n8, keys_bytes;
    __host__ __device__ PartLds(u32 key_bytes, u32 S, u32 n_words, u32 cnt32_)
        : S1(S + 1), cnt32(cnt32_), n8(n_words - (u32)__builtin_popcount(cnt32_)), keys_bytes((key_bytes * (S + 1) + 7) & ~7u)
    {
    }
    // the table's size; a kernel zeroes whole 8-byte words up to bytes() / 8 + 1 of them, so the host allocates bytes() + 16
    __host__ __device__ u32 bytes() const { return keys_bytes + 8 * S1 * n8 + 4 * S1 * (u32)__builtin_popcount(cnt32); }
    __device__ __forceinline__ u32 off(u32 w) const
    {
        const u32 low = (1u << w) - 1;
        if ((cnt32 >> w) & 1)
            return keys_bytes + 8 * S1 * n8 + 4 * S1 * (u32)__popc(cnt32 & low);
        return keys_bytes + 8 * S1 * (u32)__popc(~cnt32 & low);
    }
};

// Find-or-claim the LDS cell of `key`: linear probing from cell `start`, at most `probes` cells.  The zero key has cell S (and sets
// lzero).  Returns the cell, or ~0 when the table is full around `start`.
template <typename KT>
__device__ __forceinline__ u32 lds_find_or_claim(KT * lkeys, KT key, u32 start, int probes, u32 S, u32 & lzero)
{
    typedef typename std::conditional<sizeof(KT) == 4, unsigned int, unsigned long long>::type CasT;
    if (key == 0)
    {
        lzero = 1;
        return S;
    }
    u32 s = start;
#pragma unroll 1
    for (int probe = 0; probe < probes; ++probe)
    {
        KT k = lkeys[s];
        if (k == 0)
            k = (KT)atomicCAS((CasT *)&lkeys[s], (CasT)0, (CasT)key), k = (k == 0) ? key : k;
        if (k == key)
            return s;
        s = (s + 1) & (S - 1);
    }
    return ~0u;
}

// Flush the workgroup's LDS table into the HBM table: one emplace per occupied cell (it may use the slack above max fill) and one global
// update per state word, the high half of a fixed-point sum travelling with its low half.  Find-only mode: the cell of a key the table
// lacks goes to the overflow row s_ovf.  Every thread calls it, after a barrier.
template <typename KT>
__device__ __forceinline__ void lds_flush(const AggTable & t, const AggDesc & d, const unsigned char * lds_raw, const PartLds & L, u32 S, const u32 & lzero, u64 * s_ovf)
{
    const KT * lkeys = (const KT *)lds_raw;
    for (u32 s = threadIdx.x; s <= S; s += blockDim.x)
    {
        const u64 key = (u64)lkeys[s];
        const bool occupied = (s == S) ? (lzero != 0) : (key != 0);
        if (!occupied)
            continue;
        const u64 slot = table_place(t, s == S ? 0 : key, false);
        if (slot == ~0ull)
        {
            t.ctrl->fatal = 1;
            continue;
        }
        const bool miss = slot == AGG_SLOT_MISS;
        if (miss && !t.ovf)
            continue;
        for (u32 w = 0; w < d.words.n_words; ++w)
        {
            if ((d.words.fx_high >> w) & 1)
                continue; // flushed with its low half
            const unsigned char * wp = lds_raw + L.off(w);
            const u64 bits = ((L.cnt32 >> w) & 1) ? (u64)((const u32 *)wp)[s] : ((const u64 *)wp)[s];
            const u64 hb = ((d.words.fx >> w) & 1) ? ((const u64 *)(lds_raw + L.off(d.words.fx_hi[w])))[s] : 0;
            if (miss)
                add_cell_word(LdsRowSink{s_ovf}, d, w, bits, hb);
            else
                add_cell_word(GlobalSink(t, slot), d, w, bits, hb);
        }
    }
}

enum { AGG_MODE_ALL = 0, AGG_MODE_PENDING = 1 };

// DIRECT kernel: one global emplace + one atomic per state word per row.
template <int MODE>
__global__ __launch_bounds__(AGG_THREADS) void k_agg_rows_direct(AggTable t, AggDesc d, const void * __restrict__ keys, int key_type,
                                                                 u64 row_begin, u64 n, u64 * __restrict__ pending)
{
    __shared__ u64 s_ovf[AGG_MAX_WORDS];
    if (t.ovf)
    {
        ovf_lds_init(s_ovf);
        __syncthreads();
    }
    const u32 lane = threadIdx.x & 63;
    const u64 wave0 = ((u64)blockIdx.x * AGG_THREADS + threadIdx.x) >> 6;
    const u64 n_waves = ((u64)gridDim.x * AGG_THREADS) >> 6;
    const u64 n_groups64 = (n + 63) / 64;
    for (u64 g = wave0; g < n_groups64; g += n_waves)
    {
        const u64 r = g * 64 + lane;
        bool active = r < n;
        if (MODE == AGG_MODE_PENDING)
        {
            const u64 word = pending[g];
            if (word == 0)
                continue;
            active = active && ((word >> lane) & 1);
        }
        bool failed = false;
        if (active)
        {
            const u64 i = row_begin + r;
            failed = place_and_add(t, s_ovf, load_key_zext(keys, key_type, i), true, [&](auto sink) { add_row(sink, d, i); });
        }
        const u64 b = __ballot(failed);
        if (lane == 0)
            pending[g] = b;
        if (b != 0 && lane == 0)
            t.ctrl->overflow = 1; // benign race: every writer stores 1
    }
    if (t.ovf)
    {
        __syncthreads();
        ovf_flush_desc(t, s_ovf, d);
    }
}

// LDS-STAGED kernel.  Dynamic LDS: lkeys[S+1] then lwords[n_words][S+1]; cell S is the zero key's (PartLds with 8-byte keys and no
// 32-bit counts: the flush reads it as such).
__global__ __launch_bounds__(1024) void k_agg_rows_lds(AggTable t, AggDesc d, const void * __restrict__ keys, int key_type,
                                                              u64 row_begin, u64 n, u64 * __restrict__ pending, u32 S)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    u64 * lkeys = (u64 *)lds_raw;
    u64 * lwords = lkeys + (S + 1);
    __shared__ u32 lzero;
    __shared__ u64 s_ovf[AGG_MAX_WORDS];
    const u32 lstride = S + 1;
    for (u32 s = threadIdx.x; s < (d.words.n_words + 1) * lstride; s += blockDim.x)
        lkeys[s] = 0;
    if (threadIdx.x == 0)
        lzero = 0;
    ovf_lds_init(s_ovf);
    __syncthreads();

    const u32 lane = threadIdx.x & 63;
    // aggregate descriptors decoded once into wave-uniform registers (loops over them are fully unrolled): an s_load of d.a[j]
    // per function and row group also drains the wave's LDS queue through lgkmcnt(0) -- see k_agg_part_lds
    const void * a_ptr[AGG_MAX_AGGS];
    int a_kind[AGG_MAX_AGGS], a_type[AGG_MAX_AGGS];
    u32 a_word[AGG_MAX_AGGS], a_hi[AGG_MAX_AGGS]; // a_hi: the high word of a fixed-point sum (0 = an ordinary state word)
    int a_cond[AGG_MAX_AGGS];                     // -1: unconditioned; else (condition column << 1) | the value its non-zero test must give
    bool a_cnt2[AGG_MAX_AGGS];                    // word + 1 counts rows: avg's denominator, a NULL-mode sum's `seen`
    const int fx_base = d.fx_base;
#pragma unroll
    for (u32 j = 0; j < AGG_MAX_AGGS; ++j)
    {
        const bool on = j < d.n_aggs;
        a_ptr[j] = on ? d.a[j].ptr : nullptr;
        a_kind[j] = on ? d.a[j].kind : -1;
        a_type[j] = on ? d.a[j].arg_type : 0;
        a_word[j] = on ? d.a[j].word : 0;
        a_hi[j] = (on && d.a[j].kind != CHGPU_AGG_COUNT && ((d.words.fx >> d.a[j].word) & 1)) ? d.words.fx_hi[d.a[j].word] : 0;
        a_cond[j] = (on && d.a[j].cond >= 0) ? (d.a[j].cond << 1) | d.a[j].cond_want : -1;
        a_cnt2[j] = on && (d.a[j].kind == CHGPU_AGG_AVG || d.a[j].seen);
    }
    const u64 wave0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const u64 n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
    const u64 n_groups64 = (n + 63) / 64;
    // Each wave takes LDS_R consecutive 64-row groups per iteration and issues ALL their key/argument loads before
    // touching LDS: with one row per lane per iteration only ~24 KiB of 4-8-byte loads were in flight per CU and the
    // kernel was latency-bound (measured 18.6 -> 10.2 ms from more waves alone).
    constexpr int LDS_R = 4;
    constexpr u32 PRE = 3; // argument columns preloaded per row (further ones are loaded on use)
    for (u64 g0 = wave0 * LDS_R; g0 < n_groups64; g0 += n_waves * LDS_R)
    {
        u64 keyv[LDS_R];
        u64 argv[LDS_R][PRE];
        bool act[LDS_R];
#pragma unroll
        for (int q = 0; q < LDS_R; ++q)
        {
            const u64 r = (g0 + q) * 64 + lane;
            act[q] = r < n;
            const u64 i = row_begin + (act[q] ? r : 0);
            keyv[q] = act[q] ? load_key_zext(keys, key_type, i) : 0;
#pragma unroll
            for (u32 j = 0; j < PRE; ++j)
                argv[q][j] = (act[q] && a_kind[j] >= 0 && a_kind[j] != CHGPU_AGG_COUNT) ? load_arg_bits(a_ptr[j], a_type[j], i) : 0;
        }
#pragma unroll
        for (int q = 0; q < LDS_R; ++q)
        {
            const u64 g = g0 + q;
            if (g >= n_groups64)
                break;
            bool failed = false;
            if (act[q])
            {
                const u64 i = row_begin + g * 64 + lane;
                const u64 key = keyv[q];
                // ---- LDS emplace: linear probing, give up after 32 cells (a nearly full LDS table) -> HBM path ----
                const u32 ls = lds_find_or_claim<u64>(lkeys, key, (u32)(dev_intHash64(key) >> 40) & (S - 1), 32, S, lzero);
                if (ls != ~0u)
                {
                    const u32 nz = cond_row_bits(d, i); // (no condition column: no load)
#pragma unroll
                    for (u32 j = 0; j < AGG_MAX_AGGS; ++j)
                    {
                        if (a_kind[j] < 0)
                            break;
                        if (a_cond[j] >= 0 && ((nz >> (a_cond[j] >> 1)) & 1u) != (u32)(a_cond[j] & 1))
                            continue; // the cell is claimed, the function skips the row
                        u64 * w = lwords + a_word[j] * lstride + ls;
                        if (a_kind[j] == CHGPU_AGG_COUNT)
                            atomicAdd((unsigned long long *)w, 1ull);
                        else
                        {
                            u64 bits;
                            if (j < PRE) bits = argv[q][j < PRE ? j : 0];
                            else bits = load_arg_bits(a_ptr[j], a_type[j], i);
                            if (a_hi[j])
                                lds_add_fx(w, lwords + a_hi[j] * lstride + ls, fx_from_double(bits, fx_base));
                            else if (a_type[j] == CHGPU_F64 || a_type[j] == CHGPU_F32)
                                atomicAdd((double *)w, __longlong_as_double((long long)bits));
                            else
                                atomicAdd((unsigned long long *)w, (unsigned long long)bits);
                            if (a_cnt2[j])
                                atomicAdd((unsigned long long *)(w + lstride), 1ull);
                        }
                    }
                }
                else
                {
                    failed = place_and_add(t, s_ovf, key, true, [&](auto sink) { add_row(sink, d, i); });
                }
            }
            const u64 b = __ballot(failed);
            if (lane == 0)
                pending[g] = b;
            if (b != 0 && lane == 0)
                t.ctrl->overflow = 1;
        }
    }
    __syncthreads();

    // ---- flush the workgroup's partial states: one emplace + n_words atomics per distinct key ----
    lds_flush<u64>(t, d, lds_raw, PartLds(8, S, d.words.n_words, 0), S, lzero, s_ovf);
    if (t.ovf)
    {
        __syncthreads();
        ovf_flush_desc(t, s_ovf, d);
    }
}

// ---------------------------------------------------------------------------------------------
// PARTITIONED path for large cardinalities (config C3: 1 M groups over 1 B rows).
// Scattered device-scope atomics top out near 2e10 per second chip-wide, so one HBM atomic per row and state word caps
// the DIRECT kernel at ~1e10 rows/s whatever the bandwidth.  Instead the rows are first split by key hash into P
// partitions small enough that a partition's groups fit one workgroup's LDS table, then every partition is aggregated
// entirely in LDS by one workgroup and flushed once:
//   k_gb_hist[_wide]  per-workgroup histogram of partition ids over its contiguous row range      (key bytes read)
//   scan              exclusive scan of counts[P][G] -> exact, atomics-free write offsets
//   k_gb_scatter      per 12288-row tile (8192 / 4096 when LDS is short): LDS counting sort by partition, then coalesced run
//                     writes                                                                     (rows read, key + 8K B/row written)
//   k_gb_units        cuts partitions into work units (a hot key's partition is shared by many workgroups)
//   k_agg_part_lds    a workgroup aggregates a unit in an LDS open-addressing table and flushes it to the HBM table
// Partition buffers hold keys in 4 bytes (key types of <= 4 bytes) or 8, argument values widened to 8-byte words.
// More groups than 1024 partitions x half an LDS table: a first level with an independent hash cuts the rows into big
// partitions, each of which goes through the same passes again.
// ---------------------------------------------------------------------------------------------
#ifndef GBP_THREADS_V
#define GBP_THREADS_V 1024
#endif
#ifndef GBP_WG_PER_CU
#define GBP_WG_PER_CU 1
#endif
static constexpr u32 GBP_THREADS = GBP_THREADS_V;
static constexpr u32 GBP_MAX_P = 1024;
static constexpr u32 GBP_MAX_K = 2;

// Fibonacci hashing: one 64-bit multiply; the top bits pick the partition, bits 20.. pick the LDS cell (the full murmur
// finalizer cost ~20 VALU ops per row in three passes that turned out to be issue-bound, not HBM-bound)
static constexpr u64 GBP_MULT = 0x9E3779B97F4A7C15ull;  // partitions of the (second-level) pass that feeds the LDS aggregate
static constexpr u64 GBP_MULT1 = 0xC2B2AE3D27D4EB4Full; // first level of a two-level partitioning: an independent multiplier
__device__ __forceinline__ u64 gbp_mix(u64 key) { return key * GBP_MULT; }
__device__ __forceinline__ u32 gbp_part_of(u64 key, u32 pmask, u64 mult) { return (u32)((key * mult) >> 52) & pmask; }
// Keys of <= 4 bytes (the partition buffers hold them as u32) hash in 32 bits: one v_mul_lo_u32 instead of a 64-bit multiply
// (~5 VALU ops) in each of the three passes, which are issue-bound.  The TOP bits of key * odd pick the partition
// (mul_hi(h, P) = top log2 P bits) and the bits right below them the LDS cell: bit b of the product depends on key bits 0..b only,
// so low product bits must not be used (keys that differ in high bits only would share them).
template <typename KT>
__device__ __forceinline__ u32 gbp_part(KT key, u32 P, u64 mult)
{
    if constexpr (sizeof(KT) == 4)
        return __umulhi((u32)key * ((u32)(mult >> 32) | 1u), P);
    else
        return gbp_part_of((u64)key, P - 1, mult);
}
template <typename KT>
__device__ __forceinline__ u32 gbp_cell(KT key, u32 P, u32 S)
{
    if constexpr (sizeof(KT) == 4)
        return __umulhi((u32)key * ((u32)(GBP_MULT >> 32) | 1u) * P, S); // the partition's bits shifted out, the next log2 S bits
    else
        return (u32)(gbp_mix((u64)key) >> 20) & (S - 1); // bits disjoint from the partition id (>> 52)
}

template <typename KT>
struct GbpPartFn
{
    u32 P;
    u64 mult;
    __device__ __forceinline__ u32 operator()(KT key) const { return gbp_part<KT>(key, P, mult); }
};

struct GbpCols
{
    u32 k;                       // number of 8-byte argument words per row
    const void * src[GBP_MAX_K];
    int type[GBP_MAX_K];
    u64 * dst[GBP_MAX_K];
};

__global__ __launch_bounds__(GBP_THREADS) void k_gb_hist(const void * __restrict__ keys, int key_type, u64 row_begin, u64 n, u64 rows_per_wg,
                                                         u32 P, u32 * __restrict__ counts, u64 mult, int key32)
{
    auto part_of = [&](u64 k) -> u32 { return key32 ? gbp_part<u32>((u32)k, P, mult) : gbp_part<u64>(k, P, mult); };
    __shared__ u32 cnt[GBP_MAX_P];
    for (u32 p = threadIdx.x; p < P; p += GBP_THREADS)
        cnt[p] = 0;
    __syncthreads();
    const u64 r0 = (u64)blockIdx.x * rows_per_wg;
    const u64 r1 = r0 + rows_per_wg < n ? r0 + rows_per_wg : n;
    constexpr int HU = 8; // independent key loads in flight per lane
    u64 i = r0 + threadIdx.x;
    for (; i + (u64)(HU - 1) * GBP_THREADS < r1; i += (u64)HU * GBP_THREADS)
    {
        u64 k[HU];
#pragma unroll
        for (int q = 0; q < HU; ++q)
            k[q] = load_key_zext(keys, key_type, row_begin + i + (u64)q * GBP_THREADS);
#pragma unroll
        for (int q = 0; q < HU; ++q)
            atomicAdd(&cnt[part_of(k[q])], 1u);
    }
    for (; i < r1; i += GBP_THREADS)
        atomicAdd(&cnt[part_of(load_key_zext(keys, key_type, row_begin + i))], 1u);
    __syncthreads();
    for (u32 p = threadIdx.x; p < P; p += GBP_THREADS)
        counts[(u64)p * gridDim.x + blockIdx.x] = cnt[p];
}

// dynamic LDS: stage_word u64[K][TILE] | cursor u64[P] | delta u64[P] | stage_key KT[TILE] | tile_cnt u32[P] | tile_off u32[P]
// (the partition of a staged row is recomputed from its key in the write-out phase: one multiply instead of 2 B/row of LDS,
//  which buys a 12288-row tile -> 1.5x longer partition runs for the 4-byte-key, one-word shape)
// KT = u32 for key types of <= 4 bytes (the partition buffers then hold 4-byte keys: 12 instead of 16 B/row for C3), else u64
// WIDE: the key column is KT-wide, every argument is 8 bytes wide and the first row is 16-byte aligned in all of them;
// a thread then owns row PAIRS (tile row q*2*threads + 2*tid + {0,1}) and fetches each pair with one 8/16-byte
// nontemporal load; otherwise rows are strided by the workgroup size and loaded one by one through the type switches.
template <u32 GBP_TILE, typename KT, bool WIDE>
__global__ __launch_bounds__(GBP_THREADS) void k_gb_scatter(const void * __restrict__ keys, int key_type, u64 row_begin, u64 n, u64 rows_per_wg,
                                                            u32 P, const u64 * __restrict__ offsets, GbpCols cols, KT * __restrict__ out_keys, u64 mult)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char gb_lds[];
    u64 * stage_word = (u64 *)gb_lds;
    u64 * cursor = stage_word + (size_t)cols.k * GBP_TILE;
    u64 * delta = cursor + P; // cursor[p] - tile_off[p] of the current tile: destination row = delta[p] + position in the sorted tile
    KT * stage_key = (KT *)(delta + P);
    u32 * tile_cnt = (u32 *)(stage_key + GBP_TILE);
    u32 * tile_off = tile_cnt + P;
    __shared__ u32 wave_tot[GBP_THREADS / 64];

    for (u32 p = threadIdx.x; p < P; p += GBP_THREADS)
    {
        cursor[p] = offsets[(u64)p * gridDim.x + blockIdx.x];
        tile_cnt[p] = 0;
    }
    __syncthreads();
    const u64 r0 = (u64)blockIdx.x * rows_per_wg;
    const u64 r1 = r0 + rows_per_wg < n ? r0 + rows_per_wg : n;
    constexpr u32 RPT = GBP_TILE / GBP_THREADS; // rows per thread per tile
    // Register budget at 1024 threads is 128 VGPRs: keys are held in the buffer's key width, and the 12288-row tile -- which
    // only fits LDS with one argument word -- does not carry registers for a second one (it used to spill 9 dwords per lane)
    constexpr u32 KW = GBP_TILE >= 12288 ? 1 : GBP_MAX_K;
    KT key[RPT];
    u64 argw[RPT][KW];
    // rows of a tile are held in registers; the NEXT tile's loads are issued right after the current tile has been
    // staged to LDS, so their latency hides behind the write-out phase (one workgroup per CU: nothing else would)
    auto row_of = [&](u64 tb, u32 j) -> u64 {
        if constexpr (WIDE)
            return tb + (u64)(j >> 1) * (2 * GBP_THREADS) + 2 * threadIdx.x + (j & 1);
        else
            return tb + (u64)j * GBP_THREADS + threadIdx.x;
    };
    auto load_tile = [&](u64 tb) {
        if constexpr (WIDE)
        {
            typedef u64 v2q __attribute__((ext_vector_type(2)));
            typedef u32 v2d __attribute__((ext_vector_type(2)));
            static_assert(RPT % 2 == 0, "row pairs");
#pragma unroll
            for (u32 j = 0; j < RPT; j += 2)
            {
                const u64 i = row_of(tb, j);
                if (i + 1 < r1)
                {
                    if constexpr (sizeof(KT) == 4)
                    {
                        const v2d kk = __builtin_nontemporal_load((const v2d *)((const u32 *)keys + row_begin + i));
                        key[j] = kk.x, key[j + 1] = kk.y;
                    }
                    else
                    {
                        const v2q kk = __builtin_nontemporal_load((const v2q *)((const u64 *)keys + row_begin + i));
                        key[j] = kk.x, key[j + 1] = kk.y;
                    }
                    if (cols.k > 0)
                    {
                        const v2q a = __builtin_nontemporal_load((const v2q *)((const u64 *)cols.src[0] + row_begin + i));
                        argw[j][0] = a.x, argw[j + 1][0] = a.y;
                    }
                    if constexpr (KW > 1)
                        if (cols.k > 1)
                        {
                            const v2q a = __builtin_nontemporal_load((const v2q *)((const u64 *)cols.src[1] + row_begin + i));
                            argw[j][KW - 1] = a.x, argw[j + 1][KW - 1] = a.y;
                        }
                }
                else
                {
                    const bool in = i < r1; // at most the first row of the pair is left
                    key[j] = in ? ((const KT *)keys)[row_begin + i] : (KT)0;
                    argw[j][0] = (in && cols.k > 0) ? ((const u64 *)cols.src[0])[row_begin + i] : 0;
                    key[j + 1] = 0, argw[j + 1][0] = 0;
                    if constexpr (KW > 1)
                    {
                        argw[j][KW - 1] = (in && cols.k > 1) ? ((const u64 *)cols.src[1])[row_begin + i] : 0;
                        argw[j + 1][KW - 1] = 0;
                    }
                }
            }
        }
        else
        {
#pragma unroll
            for (u32 j = 0; j < RPT; ++j)
            {
                const u64 i = row_of(tb, j);
                const bool in = i < r1;
                key[j] = in ? (KT)load_key_zext(keys, key_type, row_begin + i) : (KT)0;
                argw[j][0] = (in && cols.k > 0) ? load_arg_bits(cols.src[0], cols.type[0], row_begin + i) : 0;
                if constexpr (KW > 1)
                    argw[j][KW - 1] = (in && cols.k > 1) ? load_arg_bits(cols.src[1], cols.type[1], row_begin + i) : 0;
            }
        }
    };
    if (r0 < r1)
        load_tile(r0);
    for (u64 tbase = r0; tbase < r1; tbase += GBP_TILE)
    {
        u32 part[RPT], rank[RPT];
        // 1. take a rank inside the tile's partition bucket
#pragma unroll
        for (u32 j = 0; j < RPT; ++j)
        {
            const u64 i = row_of(tbase, j);
            part[j] = ~0u;
            if (i < r1)
            {
                part[j] = gbp_part<KT>(key[j], P, mult);
                rank[j] = atomicAdd(&tile_cnt[part[j]], 1u);
            }
        }
        __syncthreads();
        // 2. exclusive scan of tile_cnt[P] -> tile_off[P]   (P <= 2 * threads)
        {
            const u32 e0 = threadIdx.x * 2, e1 = e0 + 1;
            u32 c0, c1;
            const u32 base = rp_scan_counters<false>(tile_cnt, P, wave_tot, c0, c1);
            // the same thread that scanned partition p also advances its cursor and clears its counter for the next tile:
            // step 1 of the next tile only starts after the barrier below, and nobody reads cursor[] again in this tile
            if (e0 < P)
            {
                tile_off[e0] = base;
                const u64 c = cursor[e0];
                delta[e0] = c - base;
                cursor[e0] = c + c0;
                tile_cnt[e0] = 0;
            }
            if (e1 < P)
            {
                tile_off[e1] = base + c0;
                const u64 c = cursor[e1];
                delta[e1] = c - (base + c0);
                cursor[e1] = c + c1;
                tile_cnt[e1] = 0;
            }
        }
        __syncthreads();
        // 3. counting sort into the LDS staging arrays
#pragma unroll
        for (u32 j = 0; j < RPT; ++j)
        {
            if (part[j] == ~0u)
                continue;
            const u32 pos = tile_off[part[j]] + rank[j];
            stage_key[pos] = (KT)key[j];
            if (cols.k > 0)
                stage_word[pos] = argw[j][0];
            if constexpr (KW > 1)
                if (cols.k > 1)
                    stage_word[(size_t)GBP_TILE + pos] = argw[j][KW - 1];
        }
        if (tbase + GBP_TILE < r1)
            load_tile(tbase + GBP_TILE); // prefetch: lands while this tile is written out
        __syncthreads();
        // 4. write the partition runs: consecutive lanes -> consecutive addresses inside a run
        const u32 tile_rows = (u32)(r1 - tbase < GBP_TILE ? r1 - tbase : GBP_TILE);
        for (u32 pos = threadIdx.x; pos < tile_rows; pos += GBP_THREADS)
        {
            const u32 p = gbp_part<KT>(stage_key[pos], P, mult);
            const u64 dst = delta[p] + pos;
            // plain stores: runs are 64-128 B, L2 write-combining completes the lines (nontemporal stores: 4.7 -> 8.1 ms)
            out_keys[dst] = stage_key[pos];
            for (u32 c = 0; c < cols.k; ++c)
                cols.dst[c][dst] = stage_word[(size_t)c * GBP_TILE + pos];
        }
        // no barrier here: the next tile's step 1 touches only tile_cnt[] (cleared in step 2 above), and its step 2 -- the
        // first writer of tile_off[]/delta[] -- sits behind the barrier that ends step 1, which every wave reaches only
        // after it has finished writing this tile out
    }
}

// Work units of the aggregate pass: partition p is cut into ceil(rows_p / chunk_rows) chunks so that a partition swollen
// by a hot key (Zipf) is shared by many workgroups instead of serialising the pass on one.  unit_start[p] = first unit of
// partition p, unit_start[P] = number of units; ctr is the dynamic work counter the workgroups draw units from.
__global__ __launch_bounds__(1024) void k_gb_units(const u64 * __restrict__ offsets, u32 G, u32 P, u64 n, u64 chunk_rows, u32 * __restrict__ unit_start, u32 * __restrict__ ctr)
{
    __shared__ u32 sc[1024];
    const u32 p = threadIdx.x;
    u32 c = 0;
    if (p < P)
    {
        const u64 begin = offsets[(u64)p * G];
        const u64 end = p + 1 < P ? offsets[(u64)(p + 1) * G] : n;
        c = (u32)((end - begin + chunk_rows - 1) / chunk_rows);
    }
    sc[p] = c;
    __syncthreads();
    for (u32 dlt = 1; dlt < 1024; dlt <<= 1)
    {
        const u32 o = p >= dlt ? sc[p - dlt] : 0;
        __syncthreads();
        sc[p] += o;
        __syncthreads();
    }
    if (p < P)
        unit_start[p] = sc[p] - c;
    if (p == P - 1)
        unit_start[P] = sc[p];
    if (p == 0)
        *ctr = 0;
}

// One workgroup aggregates whole partitions in LDS.  Partition p occupies rows [offsets[p*G], offsets[(p+1)*G]) of the
// partition buffers (n for the last).  Rows whose key cannot be placed in LDS go to the HBM table directly; rows that hit
// the max-fill limit there are marked pending (atomicOr: 64-row groups straddle partition boundaries).
//
// LDS cells are compact: the key array has the width of the partition buffer's keys (KT) and, when `cnt32` has bit w set,
// state word w is a row COUNT kept as 32 bits (a call never sees 2^32 rows; the host checks).  For the C3 shape
// (UInt32 key, sum, count) a cell is 4+8+4 = 16 B, so 8192 cells fit and 256 partitions suffice for 1 M groups --
// half as many partitions means partition runs twice as long in the scatter, whose cost is dominated by short runs.
// widening of a zero-extended narrow argument load (see ex0/ex1 in k_agg_part_lds)
__device__ __forceinline__ u64 part_extend(u64 raw, int ex)
{
    switch (ex)
    {
        case 1: return (u64)(i64)(i8)(u8)raw;
        case 2: return (u64)(i64)(i16)(u16)raw;
        case 3: return (u64)(i64)(i32)(u32)raw;
        default: return (u64)__double_as_longlong((double)__uint_as_float((u32)raw));
    }
}

// does any state word of the compile-time update code use operation a or b?  (7: the low half of a fixed-point sum of argument word 0 --
// it counts as a user of that word with 1 and 3; 9: the high half, updated together with its low half)
__host__ __device__ constexpr bool gbp_ops_use(u32 ops, u32 a, u32 b)
{
    for (u32 w = 0; w < 8; ++w)
    {
        const u32 op = (ops >> (4 * w)) & 15u;
        if (op == a || op == b || (op == 7 && (a == 1 || b == 1 || a == 3 || b == 3)))
            return true;
    }
    return false;
}
// index of the (first) state word with operation `code`
__host__ __device__ constexpr u32 gbp_ops_find(u32 ops, u32 code)
{
    for (u32 w = 0; w < 8; ++w)
        if (((ops >> (4 * w)) & 15u) == code)
            return w;
    return 0;
}

// the compile-time state update of one row at LDS cell ls: b0 / b1 = argument word 0 / 1, w_off[w] = PartLds::off(w).  (fx_base by
// reference: handed over by value, a descriptor field is fetched ahead of the walk, not where operation 7 uses it, and the 8-byte-key
// tile kernels with a fixed-point sum then need one more VGPR)
template <u32 OPS>
__device__ __forceinline__ void lds_update_ops(unsigned char * lds_raw, const u32 (&w_off)[4], u32 ls, u64 b0, u64 b1, const int & fx_base)
{
#pragma unroll
    for (u32 w = 0; w < 4; ++w)
    {
        const u32 op = (OPS >> (4 * w)) & 15u;
        if (op == 0)
            break;
        unsigned char * wp = lds_raw + w_off[w];
        if (op == 1 || op == 2)
            atomicAdd((unsigned long long *)wp + ls, (unsigned long long)(op == 1 ? b0 : b1));
        else if (op == 7)
            lds_add_fx((u64 *)wp + ls, (u64 *)(lds_raw + w_off[gbp_ops_find(OPS, 9)]) + ls, fx_from_double(b0, fx_base));
        else if (op == 9)
            continue;
        else if (op == 3 || op == 4)
            atomicAdd((double *)wp + ls, __longlong_as_double((long long)(op == 3 ? b0 : b1)));
        else if (op == 5)
            atomicAdd((unsigned int *)wp + ls, 1u);
        else
            atomicAdd((unsigned long long *)wp + ls, 1ull);
    }
}

// AW: bytes per element of the argument columns (8 in PARTITION mode -- the buffers hold widened words; 8, 4 or 1 in RANGE mode,
// where the source columns are read as they are and 4-byte signed arguments are sign-extended after the load)
// KS: element type of the key column as stored (UInt8 keys are read as they are and held as KT = UInt32 in LDS)
// EXT: some argument word of this launch needs more than the zero extension its typed load gives (Int8/16/32 sign extension,
// Float32 -> Float64); compiled out otherwise -- the pass is issue-bound and the extension logic cost it 4-14 % when present
// OPS != 0: the state update is fixed at compile time -- 4 bits per state word, word 0 in the low nibble: 1 / 2 = integer sum of
// argument word 0 / 1, 3 / 4 = Float64 sum of argument word 0 / 1, 5 = row count kept in 32 bits, 6 = row count in 64 bits.  The
// run-time descriptor walk costs ~25 scalar + ~10 vector instructions per 64 rows of a pass that is bound by instruction issue.
// FCOND (RANGE mode, OPS == 0): the functions of this pass share ONE condition column `fcond` (-If / Nullable argument): a row whose
// byte is not `fwant` (1: non-zero, 0: zero) still claims its cell -- the group exists -- and skips the update.  Compiled out otherwise.
template <typename KT, int AW, typename KS = KT, bool EXT = false, u32 OPS = 0, bool FCOND = false>
__global__ __launch_bounds__(1024) void k_agg_part_lds(AggTable t, AggDesc d, const KS * __restrict__ keys, const void * __restrict__ words0, const void * __restrict__ words1,
                                                       const u64 * __restrict__ offsets, u32 G, u32 P, u64 n, u64 * __restrict__ pending, u32 S, u32 K, u32 cnt32,
                                                       u64 rows_per_chunk, const u32 * __restrict__ unit_start, u32 * __restrict__ unit_ctr,
                                                       const u8 * __restrict__ cond, const u8 * __restrict__ fcond, u32 fwant)
{
    static_assert(!FCOND || OPS == 0, "a conditioned pass takes the generic update loop");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    KT * lkeys = (KT *)lds_raw;
    const PartLds L((u32)sizeof(KT), S, d.words.n_words, cnt32);
    const u32 lds_bytes = L.bytes();
    __shared__ u32 lzero, sh_unit;
    __shared__ u64 s_ovf[AGG_MAX_WORDS]; // find-only mode: the workgroup's share of the overflow row (made visible by the loop's first barrier)
    ovf_lds_init(s_ovf);
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    // The aggregate descriptors are decoded ONCE into wave-uniform registers (all loops over them are fully unrolled, so the
    // indices are constants): fetching d.a[j] inside the row loop meant an s_load per function and row group, and its
    // s_waitcnt lgkmcnt(0) also drains every LDS operation the wave has in flight -- the pass was issue-bound at ~170
    // clocks per 64 rows while the LDS itself can take this mix at 8.5 lanes/clock (tools/lds_bench.hip).
    //   op: 0 none, 1 add u64 (integer sum), 2 add f64, 3 count as u32, 4 count as u64
    u32 a_off[AGG_MAX_AGGS], a_off2[AGG_MAX_AGGS], a_off3[AGG_MAX_AGGS];
    int a_op[AGG_MAX_AGGS], a_op2[AGG_MAX_AGGS], a_src[AGG_MAX_AGGS];
    const int fx_base = d.fx_base;
    // what to do with the zero-extended load of argument word 0 / 1: 0 nothing, 1/2/3 sign-extend from 8/16/32 bits (Int8/16/32
    // columns), 4 Float32 -> Float64 bits
    int ex0 = 0, ex1 = 0;
#pragma unroll
    for (u32 j = 0; j < AGG_MAX_AGGS; ++j)
    {
        a_off[j] = a_off2[j] = a_off3[j] = 0;
        a_op[j] = a_op2[j] = a_src[j] = 0;
        if (OPS == 0 && j < d.n_aggs)
        {
            const u32 w = d.a[j].word;
            a_off[j] = L.off(w);
            if (d.a[j].kind == CHGPU_AGG_COUNT)
                a_op[j] = ((cnt32 >> w) & 1) ? 3 : 4;
            else
            {
                a_op[j] = (d.a[j].arg_type == CHGPU_F64 || d.a[j].arg_type == CHGPU_F32) ? 2 : 1;
                if ((d.words.fx >> w) & 1)
                {
                    a_op[j] = 5; // 128-bit fixed-point sum: the low half at a_off, the high half at a_off3
                    a_off3[j] = L.off(d.words.fx_hi[w]);
                }
                a_src[j] = (int)d.a[j].pre;
                const int ex = d.a[j].arg_type == CHGPU_I8 ? 1 : d.a[j].arg_type == CHGPU_I16 ? 2 : d.a[j].arg_type == CHGPU_I32 ? 3 : d.a[j].arg_type == CHGPU_F32 ? 4 : 0;
                (d.a[j].pre == 0 ? ex0 : ex1) = ex;
                if (d.a[j].kind == CHGPU_AGG_AVG || d.a[j].seen) // avg's denominator; a NULL-mode sum's `seen` word
                {
                    a_off2[j] = L.off(w + 1);
                    a_op2[j] = ((cnt32 >> (w + 1)) & 1) ? 3 : 4;
                }
            }
        }
    }
    u32 w_off[4];
#pragma unroll
    for (u32 w = 0; w < 4; ++w)
        w_off[w] = L.off(w);
    // PARTITION mode: work units (partition, chunk) are drawn from a device-wide counter until it passes the unit count
    // (every workgroup reaches that exit).  RANGE mode (offsets == nullptr): chunk blockIdx.x, +gridDim.x, ... of the
    // source columns themselves (keys/words0/words1 point at the block's first row) -- the low-cardinality GROUP BY runs this way.
    const u32 n_units = offsets ? unit_start[P] : P;
    for (u32 iter = 0;; ++iter)
    {
        u32 unit;
        if (offsets)
        {
            if (threadIdx.x == 0)
                sh_unit = atomicAdd(unit_ctr, 1u);
            __syncthreads();
            unit = sh_unit;
        }
        else
            unit = blockIdx.x + iter * gridDim.x;
        if (unit >= n_units)
            break;
        u64 begin, end;
        if (offsets)
        {
            u32 lo = 0, hi = P - 1; // largest p with unit_start[p] <= unit
            while (lo < hi)
            {
                const u32 mid = (lo + hi + 1) >> 1;
                if (unit_start[mid] <= unit)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            const u32 p = lo;
            const u64 pbegin = offsets[(u64)p * G];
            const u64 pend = p + 1 < P ? offsets[(u64)(p + 1) * G] : n;
            begin = pbegin + (u64)(unit - unit_start[p]) * rows_per_chunk;
            end = begin + rows_per_chunk < pend ? begin + rows_per_chunk : pend;
        }
        else
        {
            begin = (u64)unit * rows_per_chunk;
            end = begin + rows_per_chunk < n ? begin + rows_per_chunk : n;
        }
        for (u32 s = threadIdx.x; s < lds_bytes / 8 + 1; s += blockDim.x)
            ((u64 *)lds_raw)[s] = 0; // the host rounds the allocation up to 8 bytes past lds_bytes
        if (threadIdx.x == 0)
            lzero = 0;
        __syncthreads();
        const u64 g0 = begin / 64, g1 = (end + 63) / 64;
        constexpr int PR = 4;  // 64-row groups per wave iteration: all their loads are issued before LDS is touched
        constexpr u32 PPRE = 2; // argument words preloaded per row (GBP_MAX_K)
        // Loads are unconditional (row indices clamped to the buffer) and double-buffered in registers: the loads of the
        // wave's next PR groups are in flight while the current ones go through the LDS table.  No branch surrounds a
        // load, so the compiler can keep exact vmcnt waits instead of draining the queue at a control-flow join.
        // cond (RANGE mode only): the WHERE mask of a fused filter + GROUP BY; rows whose byte is 0 are skipped entirely, as if a
        // FilterTransform had removed them before the AggregatingTransform.
        auto load_set = [&](u64 gb, u64 (&kv)[PR], u64 (&av)[PR][PPRE], u32 (&cv)[PR]) {
#pragma unroll
            for (int q = 0; q < PR; ++q)
            {
                u64 i = (gb + q) * 64 + lane;
                i = i < n ? i : n - 1;
                cv[q] = cond ? (u32)__builtin_nontemporal_load(&cond[i]) : 1u;
                if constexpr (FCOND) // bit 8: the row reaches the pass's functions (the WHERE byte stays in the low bits)
                    cv[q] = (cv[q] & 0xffu) | ((u32)((u32)(__builtin_nontemporal_load(&fcond[i]) != 0) == fwant) << 8);
                kv[q] = (u64)__builtin_nontemporal_load(&keys[i]);
                typedef typename std::conditional<AW == 8, u64, typename std::conditional<AW == 4, u32, typename std::conditional<AW == 2, u16, u8>::type>::type>::type AT;
                // (with a compile-time OPS the loads are unconditional or absent: a run-time `K > 0` puts a branch around each load)
                if constexpr (OPS != 0)
                {
                    av[q][0] = gbp_ops_use(OPS, 1, 3) ? (u64)__builtin_nontemporal_load((const AT *)words0 + i) : 0;
                    av[q][1] = gbp_ops_use(OPS, 2, 4) ? (u64)__builtin_nontemporal_load((const AT *)words1 + i) : 0;
                }
                else
                {
                    av[q][0] = K > 0 ? (u64)__builtin_nontemporal_load((const AT *)words0 + i) : 0;
                    av[q][1] = K > 1 ? (u64)__builtin_nontemporal_load((const AT *)words1 + i) : 0;
                }
            }
        };
        // (Combining the rows of a hot key in registers before the LDS atomic was tried for Zipf inputs: once partitions are
        //  cut into work units it gains nothing -- 15.2 ms without vs 14.9-15.7 ms with -- and costs the uniform case 3-10 %.)
        auto process_set = [&](u64 gb, const u64 (&keyv)[PR], const u64 (&argv)[PR][PPRE], const u32 (&cv)[PR]) {
#pragma unroll
            for (int q = 0; q < PR; ++q)
            {
                const u64 g = gb + q;
                if (g >= g1)
                    break;
                const u64 i = g * 64 + lane;
                bool failed = false;
                if (i >= begin && i < end && (FCOND ? (cv[q] & 0xffu) : cv[q]) != 0)
                {
                    const bool reached = !FCOND || (cv[q] >> 8) != 0;
                    const u64 key = keyv[q];
                    u64 b0 = argv[q][0], b1 = argv[q][1];
                    if constexpr (EXT)
                    {
                        if (ex0) // wave-uniform
                            b0 = part_extend(b0, ex0);
                        if (ex1)
                            b1 = part_extend(b1, ex1);
                    }
                    // (start cell: bits disjoint from the partition id)
                    const u32 ls = lds_find_or_claim<KT>(lkeys, (KT)key, gbp_cell<KT>((KT)key, offsets ? P : 1u, S), 64, S, lzero);
                    if (ls != ~0u)
                    {
                        if constexpr (OPS != 0)
                            lds_update_ops<OPS>(lds_raw, w_off, ls, b0, b1, fx_base);
                        else
#pragma unroll
                        for (u32 j = 0; j < AGG_MAX_AGGS; ++j)
                        {
                            if (a_op[j] == 0 || !reached)
                                break;
                            unsigned char * w = lds_raw + a_off[j];
                            const u64 bits = a_src[j] == 0 ? b0 : b1;
                            if (a_op[j] == 1)
                                atomicAdd((unsigned long long *)w + ls, (unsigned long long)bits);
                            else if (a_op[j] == 2)
                                atomicAdd((double *)w + ls, __longlong_as_double((long long)bits));
                            else if (a_op[j] == 3)
                                atomicAdd((unsigned int *)w + ls, 1u);
                            else if (a_op[j] == 5)
                                lds_add_fx((u64 *)w + ls, (u64 *)(lds_raw + a_off3[j]) + ls, fx_from_double(bits, fx_base));
                            else
                                atomicAdd((unsigned long long *)w + ls, 1ull);
                            if (a_op2[j] == 3)
                                atomicAdd((unsigned int *)(lds_raw + a_off2[j]) + ls, 1u); // avg's denominator
                            else if (a_op2[j] == 4)
                                atomicAdd((unsigned long long *)(lds_raw + a_off2[j]) + ls, 1ull);
                        }
                    }
                    else
                    {
                        failed = place_and_add(t, s_ovf, key, true, [&](auto sink) {
                            if (reached)
                                add_vals(sink, d, b0, b1, 1);
                        });
                    }
                }
                const u64 b = __ballot(failed);
                if (b != 0 && lane == 0)
                {
                    atomicOr((unsigned long long *)&pending[g], (unsigned long long)b);
                    t.ctrl->overflow = 1;
                }
            }
        };
        {
            const u64 step = (u64)n_waves * PR;
            u64 kA[PR], aA[PR][PPRE], kB[PR], aB[PR][PPRE];
            u32 cA[PR], cB[PR];
            u64 gb = g0 + (u64)wave * PR;
            load_set(gb, kA, aA, cA);
            for (; gb < g1; gb += 2 * step)
            {
                load_set(gb + step, kB, aB, cB);
                __builtin_amdgcn_sched_barrier(0);
                process_set(gb, kA, aA, cA);
                load_set(gb + 2 * step, kA, aA, cA);
                __builtin_amdgcn_sched_barrier(0);
                process_set(gb + step, kB, aB, cB);
            }
        }
        __syncthreads();
        lds_flush<KT>(t, d, lds_raw, L, S, lzero, s_ovf);
        __syncthreads();
    }
    if (t.ovf) // (the loop ends on a barrier)
        ovf_flush_desc(t, s_ovf, d);
}

// ---- the TILE-SORTED plan (radix_partition.h, k_rp_tilesort): units and the aggregate pass that gathers one run per tile ----
// A partition of r rows gets c = ceil(r / chunk_rows) units, unit (p, j) = the j-th of c equal shares of the TILES (a partition swollen
// by a hot key is long in every tile, so cutting by tiles cuts its rows evenly).  unit_list is ordered by (j, p): the workgroups draw
// units in that order, so at any time they work on the SAME stretch of tiles for different partitions -- the lines at the two ends of
// a run also hold the neighbouring partitions' rows and are then found in L2 / Infinity Cache by the neighbours instead of being
// fetched from HBM once per partition.  unit_list[u] = p | j << 16 | c << 40; unit_count[0] = number of units.
static constexpr u32 TILE_QUEUES = 8; // XCDs of an MI355X
__global__ __launch_bounds__(1024) void k_tile_units(const unsigned long long * __restrict__ part_total, u32 P, u64 chunk_rows, u32 n_tiles, u64 * __restrict__ unit_list,
                                                      u32 max_units, u32 * __restrict__ qstart, u32 * __restrict__ ctr)
{
    __shared__ u32 sc[1024], cc[1024];
    const u32 p = threadIdx.x;
    u32 c = 0;
    if (p < P)
    {
        const u64 c64 = (part_total[p] + chunk_rows - 1) / chunk_rows;
        c = (u32)(c64 < n_tiles ? c64 : n_tiles); // a unit is at least one tile
    }
    sc[p] = c;
    cc[p] = c;
    __syncthreads();
    for (u32 dlt = 1; dlt < 1024; dlt <<= 1)
    {
        const u32 o = p >= dlt ? sc[p - dlt] : 0;
        __syncthreads();
        sc[p] += o;
        __syncthreads();
    }
    // Eight queues, one per XCD: queue x holds the units of partitions [x * PX, (x + 1) * PX) in (j, p) order, so that the 32
    // workgroups of an XCD sweep the same tiles for 32 NEIGHBOURING partitions -- the shared boundary lines are then L2 hits, not
    // just Infinity Cache hits.  (the host sized the list for the bound sum ceil(r_p / chunk) <= n / chunk + P)
    const u32 PX = (P + TILE_QUEUES - 1) / TILE_QUEUES;
    const u32 U = sc[1023] < max_units ? sc[1023] : max_units;
    for (u32 u = threadIdx.x; u < U; u += 1024)
    {
        u32 lo = 0, hi = P - 1; // the partition whose units [sc[q] - cc[q], sc[q]) hold u
        while (lo < hi)
        {
            const u32 mid = (lo + hi) >> 1;
            if (sc[mid] > u)
                hi = mid;
            else
                lo = mid + 1;
        }
        const u32 q = lo, j = u - (sc[q] - cc[q]);
        const u32 x = q / PX, r0 = x * PX, r1 = r0 + PX < P ? r0 + PX : P;
        u32 pos = r0 ? sc[r0 - 1] : 0; // the queue's first unit: all units of the partitions before it
        for (u32 r = r0; r < r1; ++r) // units of the queue ordered before (j, q): every (j', .) with j' < j, and (j, q') with q' < q
            pos += (cc[r] < j ? cc[r] : j) + ((r < q && cc[r] > j) ? 1u : 0u);
        if (pos < max_units)
            unit_list[pos] = (u64)q | ((u64)j << 16) | ((u64)cc[q] << 40);
    }
    if (p <= TILE_QUEUES)
    {
        const u32 r0 = p * PX < P ? p * PX : P;
        const u32 first = r0 ? sc[r0 - 1] : 0;
        qstart[p] = first < U ? first : U;
    }
    if (p < TILE_QUEUES)
        ctr[p] = 0;
}

// The tile index transposed for the aggregate pass: run_index[p][t] = start | length << 16 of partition p's run in tile t, so that a
// wave reads the entries of 64 consecutive tiles as ONE 256-byte load (read straight from tile_index[t][p] every entry costs a
// 128-byte line of its own: one line in seven of the whole pass).  84 MB for 1e9 rows: ~30 us.
__global__ __launch_bounds__(256) void k_tile_index_transpose(const unsigned short * __restrict__ tile_index, u32 n_tiles, u32 P, u32 * __restrict__ run_index)
{
    __shared__ u32 sm[64][65];
    const u32 tb = blockIdx.x * 64, pb = blockIdx.y * 64;
    const u32 x = threadIdx.x & 63, y0 = threadIdx.x >> 6;
    for (u32 y = y0; y < 64; y += 4) // tile tb + y, partition pb + x: consecutive lanes -> consecutive u16 entries
    {
        const u32 t = tb + y, pp = pb + x;
        u32 v = 0;
        if (t < n_tiles && pp < P)
        {
            const u32 a = tile_index[(u64)t * (P + 1) + pp], b = tile_index[(u64)t * (P + 1) + pp + 1];
            v = a | ((b - a) << 16);
        }
        sm[y][x] = v;
    }
    __syncthreads();
    for (u32 y = y0; y < 64; y += 4) // partition pb + y, tile tb + x: consecutive lanes -> consecutive tiles
    {
        const u32 t = tb + x, pp = pb + y;
        if (t < n_tiles && pp < P)
            run_index[(u64)pp * n_tiles + t] = sm[x][y];
    }
}

// A block of 64 entries of run_index, lane l <- the wave's tile ordinal kb + l (kb a multiple of 64: 64 consecutive tiles starting at
// `first`), 0 beyond the unit's last tile t1.
__device__ __forceinline__ u32 tiles_load_block(const u32 * __restrict__ run_index_p, u32 first, u32 t1, u32 lane)
{
    const u32 tl = first + lane;
    const bool valid = tl < t1;
    const u32 v = run_index_p[valid ? tl : t1 - 1];
    return valid ? v : 0u;
}

// One workgroup aggregates a unit = (partition p, a range of tiles) in the same compact LDS table as k_agg_part_lds (PartLds), then
// flushes it into the HBM table.  Wave w of the workgroup takes the unit's tiles w, w + 16, w + 32, ...: the index entries (start,
// length of partition p's run) of its next 64 tiles are fetched by ONE vector load (lane l = the l-th of those tiles) into a register
// block, two blocks alternate; a step takes PR tiles: their entries come out of the block by v_readlane (wave-uniform, so the row
// addresses are scalar base + lane), their rows are loaded (lanes beyond the run's length idle: a uniform input gives runs of
// TILE / P = 48 rows) and the previous step's rows go through the LDS table meanwhile.  Runs longer than 64 rows (skewed keys) are
// finished by a plain loop after the pipelined one.
// tile_index: u16 [n_tiles][P + 1]; the two entries of (tile, p) are read as one unaligned 32-bit load.
// OPS: the compile-time state update code of k_agg_part_lds (one argument word: operations 1, 3, 5, 6).
// The sorted copy is k_rp_tilesort's array of {word, key} records: 12 bytes for 4-byte keys, 16 for 8-byte keys (words0 = its base;
// `keys` is not read).
template <typename KT, u32 OPS, u32 TILE>
__global__ __launch_bounds__(1024) void k_agg_tiles_lds(AggTable t, AggDesc d, const KT * __restrict__ keys, const u64 * __restrict__ words0,
                                                        const u32 * __restrict__ run_index, u32 n_tiles, u32 P, u64 * __restrict__ pending, u32 S, u32 cnt32,
                                                        const u64 * __restrict__ unit_list, const u32 * __restrict__ qstart, u32 * __restrict__ qctr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    KT * lkeys = (KT *)lds_raw;
    const PartLds L((u32)sizeof(KT), S, d.words.n_words, cnt32);
    const u32 lds_bytes = L.bytes();
    __shared__ u32 lzero, sh_unit;
    __shared__ u64 s_ovf[AGG_MAX_WORDS]; // find-only mode: the workgroup's share of the overflow row (made visible by the loop's first barrier)
    ovf_lds_init(s_ovf);
    const u32 lane = threadIdx.x & 63;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = blockDim.x >> 6;
    const u64 last_row = (u64)n_tiles * TILE - 1;
    u32 w_off[4];
#pragma unroll
    for (u32 w = 0; w < 4; ++w)
        w_off[w] = L.off(w);
    // units are drawn from the queue of this workgroup's XCD first (HW_REG_XCC_ID only steers the choice: when a queue runs dry the
    // workgroup goes on with the next one, so every unit is taken whatever the placement)
    const u32 xcc = __builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20) & (TILE_QUEUES - 1);
    u32 dry = 0; // (thread 0) queues found empty
    for (;;)
    {
        if (threadIdx.x == 0)
        {
            u32 got = ~0u;
            for (u32 a = 0; a < TILE_QUEUES && got == ~0u; ++a)
            {
                const u32 y = (xcc + a) & (TILE_QUEUES - 1);
                if ((dry >> y) & 1u)
                    continue;
                const u32 len = qstart[y + 1] - qstart[y];
                const u32 k = len ? atomicAdd(&qctr[y], 1u) : len;
                if (k < len)
                    got = qstart[y] + k;
                else
                    dry |= 1u << y;
            }
            sh_unit = got;
        }
        __syncthreads();
        const u32 unit = sh_unit;
        if (unit == ~0u)
            break; // (every workgroup reaches this exit: all queues are dry)
        const u64 ud = unit_list[unit];
        const u32 p = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(ud & 0xffffu)), j = (u32)__builtin_amdgcn_readfirstlane((int)(u32)((ud >> 16) & 0xffffffu)),
                  c_p = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(ud >> 40));
        const u32 t0 = (u32)((u64)n_tiles * j / c_p), t1 = (u32)((u64)n_tiles * (j + 1) / c_p);
        for (u32 s = threadIdx.x; s < lds_bytes / 8 + 1; s += blockDim.x)
            ((u64 *)lds_raw)[s] = 0; // the host rounds the allocation up to 8 bytes past lds_bytes
        if (threadIdx.x == 0)
            lzero = 0;
        __syncthreads();
        constexpr u32 PR = 8; // tiles (= runs of partition p) per wave and step
        constexpr u32 NS = 7; // 64-row slots the PR runs of a step are packed into: PR x 48 rows on average, 7 x 64 = 448 slots
        // This wave's tiles: blocks of 64 consecutive tiles, block w, w + n_waves, ... of the unit; ordinal k -> tile
        // t0 + ((k >> 6) * n_waves + wave) * 64 + (k & 63), beyond t1 = no tile.
        const u32 n_blocks = (t1 - t0 + 63) / 64;
        const u32 my_blocks = wave < n_blocks ? (n_blocks - wave + n_waves - 1) / n_waves : 0;
        const u32 ns = my_blocks * (64 / PR);
        const u32 * __restrict__ run_index_p = run_index + (u64)p * n_tiles;
        auto tile_of = [&](u32 k) -> u32 { return t0 + ((k >> 6) * n_waves + wave) * 64 + (k & 63u); };
        u32 blk0 = tiles_load_block(run_index_p, tile_of(0), t1, lane), blk1 = tiles_load_block(run_index_p, tile_of(64), t1, lane);
        // A step's PR runs are PACKED: virtual row v = slot * 64 + lane belongs to the run r with cs[r] <= v < cs[r + 1] (cs = running
        // sum of the run lengths, wave-uniform) and sits at row v + dl[r] of the sorted copy (dl[r] = tile * TILE + start - cs[r], modulo
        // 2^32: the host keeps this plan below 2^32 rows).  Runs of 48 +- 7 rows fill 86 % of the lanes instead of 75 %, and a single
        // long run borrows the slack of its neighbours; only a step with more than NS * 64 rows (skewed keys) takes the plain loop.
        auto row_of = [&](u32 v, const u32 (&cs)[PR + 1], const u32 (&dl)[PR]) -> u32 {
            // (a sum of masked steps, not a chain of selects: the compiler turns the chain into a look-up in a stack copy of dl[])
            u32 i = v + dl[0];
#pragma unroll
            for (u32 r = 1; r < PR; ++r)
                i += v >= cs[r] ? dl[r] - dl[r - 1] : 0u;
            return i;
        };
        // the LDS update of one row; the row is virtual row v of the step (PACKED_ = true_type) or row v of the sorted copy itself; its index is only needed when the LDS table is full
        auto update_row = [&](KT key, u64 b0, u32 v, auto packed, const u32 (&cs)[PR + 1], const u32 (&dl)[PR]) {
            // (start cell: bits disjoint from the partition id)
            const u32 ls = lds_find_or_claim<KT>(lkeys, key, gbp_cell<KT>(key, P, S), 64, S, lzero);
            if (ls != ~0u)
                lds_update_ops<OPS>(lds_raw, w_off, ls, b0, 0, d.fx_base); // (this kernel's operations never read argument word 1)
            else
            {
                // the LDS table is full around this key's cell (more groups than promised): the row is left to the finish rounds, which
                // send pending rows through the HBM table (kept out of this loop: the copies of the row update must stay small)
                const u64 i = decltype(packed)::value ? row_of(v, cs, dl) : v;
                atomicOr((unsigned long long *)&pending[i >> 6], 1ull << (i & 63));
                t.ctrl->overflow = 1;
            }
        };
        // step s: its PR index entries out of the blocks (crossing into a new block refills the other one), then its row loads
        auto fetch = [&](u32 s, u32 (&cs)[PR + 1], u32 (&dl)[PR], KT (&kv)[NS], u64 (&av)[NS]) {
            const u32 k0 = s * PR;
            // (the blocks are handled as values: a `cond ? blk1 : blk0` on the captured variables becomes a select of their ADDRESSES and
            //  pins the whole closure to scratch memory)
            u32 b0v = blk0, b1v = blk1;
            if ((k0 & 63u) == 0 && k0 != 0)
            {
                const u32 nb = tiles_load_block(run_index_p, tile_of(k0 + 64), t1, lane);
                const bool odd = ((k0 >> 6) & 1u) != 0;
                b0v = odd ? nb : b0v;
                b1v = odd ? b1v : nb;
                blk0 = b0v;
                blk1 = b1v;
            }
            const u32 cur = ((k0 >> 6) & 1u) ? b1v : b0v; // (PR divides 64: a step never straddles two blocks)
            u32 c = 0;
#pragma unroll
            for (u32 r = 0; r < PR; ++r)
            {
                const u32 k = k0 + r;
                const u32 ix = (u32)__builtin_amdgcn_readlane((int)cur, (int)(k & 63u));
                const u32 tl = tile_of(k);
                cs[r] = c;
                dl[r] = (tl < n_tiles ? tl : n_tiles - 1) * TILE + (ix & 0xffffu) - c;
                c += ix >> 16;
            }
            cs[PR] = c;
#pragma unroll
            for (u32 m = 0; m < NS; ++m)
            {
                u32 i = row_of(m * 64 + lane, cs, dl);
                i = i < (u32)last_row ? i : (u32)last_row; // (the lanes beyond the step's rows computed anything)
                if constexpr (sizeof(KT) == 4)
                {
                    // (the word as ONE 8-byte load from its 4-byte aligned place: combining two loaded halves is an operation on the
                    //  loaded registers, which the scheduler puts right behind the loads -- and the wave then waits for them there)
                    typedef u64 u64_a4 __attribute__((aligned(4)));
                    const u32 * r = (const u32 *)words0 + (u64)i * 3;
                    av[m] = gbp_ops_use(OPS, 1, 3) ? (u64)__builtin_nontemporal_load((const u64_a4 *)r) : 0;
                    kv[m] = (KT)__builtin_nontemporal_load(r + 2);
                }
                else
                {
                    typedef u64 v2q __attribute__((ext_vector_type(2)));
                    const v2q rec = __builtin_nontemporal_load((const v2q *)words0 + i); // {word, key}
                    av[m] = rec.x;
                    kv[m] = (KT)rec.y;
                }
            }
        };
        auto process = [&](const u32 (&cs)[PR + 1], const u32 (&dl)[PR], const KT (&kv)[NS], const u64 (&av)[NS]) {
            const u32 total = cs[PR];
#pragma unroll
            for (u32 m = 0; m < NS; ++m)
            {
                const u32 v = m * 64 + lane;
                if (v < total)
                    update_row(kv[m], av[m], v, std::true_type{}, cs, dl);
            }
            if (total > NS * 64) // (wave-uniform) skewed keys: the rest of the step's rows, unpipelined
#pragma unroll 1
                for (u32 v = NS * 64 + lane; v < total; v += 64)
                {
                    const u32 i = row_of(v, cs, dl);
                    if constexpr (sizeof(KT) == 4)
                    {
                        const u32 * r = (const u32 *)words0 + (u64)i * 3;
                        update_row((KT)r[2], gbp_ops_use(OPS, 1, 3) ? (u64)r[0] | ((u64)r[1] << 32) : 0, i, std::false_type{}, cs, dl);
                    }
                    else
                        update_row((KT)words0[2 * (u64)i + 1], words0[2 * (u64)i], i, std::false_type{}, cs, dl);
                }
        };
        {
            u32 csA[PR + 1], dlA[PR], csB[PR + 1], dlB[PR];
            KT kA[NS], kB[NS];
            u64 aA[NS], aB[NS];
            fetch(0, csA, dlA, kA, aA);
            for (u32 s = 0; s < ns; s += 2)
            {
                fetch(s + 1, csB, dlB, kB, aB);
                __builtin_amdgcn_sched_barrier(0);
                process(csA, dlA, kA, aA);
                fetch(s + 2, csA, dlA, kA, aA);
                __builtin_amdgcn_sched_barrier(0);
                process(csB, dlB, kB, aB);
            }
        }
        __syncthreads();
        lds_flush<KT>(t, d, lds_raw, L, S, lzero, s_ovf);
        __syncthreads();
    }
    if (t.ovf) // (the loop ends on a barrier)
        ovf_flush_desc(t, s_ovf, d);
}

// The finish rounds of the tile-sorted plan over 12-byte records: the rows k_agg_tiles_lds left pending (LDS table full) go through the
// HBM table; a row that meets the max-fill limit stays pending for the next round (after the table has grown).
__global__ __launch_bounds__(AGG_THREADS) void k_agg_tiles_pending_aos(AggTable t, AggDesc d, const u32 * __restrict__ rec, int key64, u64 n, u64 * __restrict__ pending)
{
    __shared__ u64 s_ovf[AGG_MAX_WORDS];
    if (t.ovf)
    {
        ovf_lds_init(s_ovf);
        __syncthreads();
    }
    const u32 lane = threadIdx.x & 63;
    const u64 wave0 = ((u64)blockIdx.x * AGG_THREADS + threadIdx.x) >> 6;
    const u64 n_waves = ((u64)gridDim.x * AGG_THREADS) >> 6;
    const u64 n_groups64 = (n + 63) / 64;
    for (u64 g = wave0; g < n_groups64; g += n_waves)
    {
        const u64 word = pending[g];
        if (word == 0)
            continue;
        const u64 i = g * 64 + lane;
        bool failed = false;
        if (i < n && ((word >> lane) & 1))
        {
            const u32 * r = rec + i * (key64 ? 4 : 3); // records are {word, key}: 12 bytes with a 4-byte key, 16 with an 8-byte key
            failed = place_and_add(t, s_ovf, key64 ? (u64)r[2] | ((u64)r[3] << 32) : (u64)r[2], true,
                                   [&](auto sink) { add_vals(sink, d, (u64)r[0] | ((u64)r[1] << 32), 0, 1); });
        }
        const u64 b = __ballot(failed);
        if (lane == 0)
            pending[g] = b;
        if (b != 0 && lane == 0)
            t.ctrl->overflow = 1;
    }
    if (t.ovf)
    {
        __syncthreads();
        ovf_flush_desc(t, s_ovf, d);
    }
}

// Merge (key, state words) tuples into the table: mergeToViaEmplace, also the rehash of a grown table.
// src_words[w] + i*1 ; src keys are u64; key==0 entries are skipped when skip_zero_keys (table arrays: empty cells),
// zero_slot_index: index in the source arrays of the out-of-line zero key (or ~0).  rehash: the tuples are the cells of the table
// being replaced: every key once, into an empty table.
// source tuple i's state words into the group's state in `sink` (table words: a merge has no word map)
template <typename Sink>
__device__ __forceinline__ void merge_tuple_words(const Sink & sink, const AggMergeWords & ws, u32 rehash, const u64 * __restrict__ src_words, u64 src_stride, u64 i)
{
    for (u32 w = 0; w < ws.n_words; ++w)
    {
        if ((ws.fx_high >> w) & 1)
            continue; // merged with its low half
        const u64 v = src_words[(u64)w * src_stride + i];
        if ((ws.any >> w) & 1)
        {
            // any(): changeFirstTime (SingleValueData.cpp) -- a state that has a value keeps it; {claim, value} move together
            if (v && atomicCAS((unsigned long long *)sink.at(w), 0ull, (unsigned long long)v) == 0ull)
                *sink.at(w + 1) = src_words[(u64)(w + 1) * src_stride + i];
            ++w;
            continue;
        }
        if ((ws.arg >> w) & 1)
        {
            const u64 has = src_words[(u64)(w + 1) * src_stride + i];
            if (rehash)
            {
                // {val, claim, arg} move unchanged: a claim may be the sentinel of a block whose claim pass is still to come
                *sink.at(w) = v;
                *sink.at(w + 1) = has;
                *sink.at(w + 2) = src_words[(u64)(w + 2) * src_stride + i];
            }
            else if (has) // (a state without a value loses every merge); claim and arg: k_agg_arg_tuples
                sink.raise(sink.at(w), sink.at(w + 1), v, AGG_MERGE_SENTINEL);
            w += 2;
            continue;
        }
        if ((ws.fx >> w) & 1)
        {
            const u32 wh = ws.fx_hi[w];
            sink.add_fx(sink.at(w), sink.at(wh), Fx128{v, src_words[(u64)wh * src_stride + i]});
            continue;
        }
        sink.add_word(sink.at(w), v, ws.op(w));
    }
}
template <int MODE>
__global__ __launch_bounds__(AGG_THREADS) void k_agg_tuples(AggTable t, AggMergeWords ws, u32 rehash, const u64 * __restrict__ src_keys,
                                                            const u64 * __restrict__ src_words, u64 src_stride, u64 n, int skip_zero_keys,
                                                            u64 zero_slot_index, int soft_limit, u64 * __restrict__ pending)
{
    const u32 lane = threadIdx.x & 63;
    const u64 wave0 = ((u64)blockIdx.x * AGG_THREADS + threadIdx.x) >> 6;
    const u64 n_waves = ((u64)gridDim.x * AGG_THREADS) >> 6;
    const u64 n_groups64 = (n + 63) / 64;
    __shared__ u64 s_ovf[AGG_MAX_WORDS]; // find-only merges (never the rehash): the workgroup's share of the overflow row
    if (t.ovf)
    {
        ovf_lds_init(s_ovf);
        __syncthreads();
    }
    u32 my_claims = 0; // without a soft limit nobody reads the counter mid-kernel: count in registers, add once per wave
    for (u64 g = wave0; g < n_groups64; g += n_waves)
    {
        const u64 i = g * 64 + lane;
        bool active = i < n;
        if (MODE == AGG_MODE_PENDING)
        {
            const u64 word = pending[g];
            if (word == 0)
                continue;
            active = active && ((word >> lane) & 1);
        }
        bool failed = false;
        if (active)
        {
            u64 key = src_keys[i];
            const bool is_zero_cell = (i == zero_slot_index);
            if (is_zero_cell)
                key = 0;
            if (!(skip_zero_keys && key == 0 && !is_zero_cell))
            {
                bool claimed = false;
                const u64 slot = t.find_only ? table_find(t, key) : table_emplace_impl(t, key, soft_limit != 0, claimed);
                if (t.find_only)
                    ;
                else if (soft_limit)
                    count_claim(t, claimed); // the only divergent caller: count_claim's ballot sees the lanes in this branch
                else
                    my_claims += claimed;
                if (slot == ~0ull)
                    failed = true;
                else if (slot == AGG_SLOT_MISS)
                {
                    // mergeDataNoMoreKeysImpl: the source state of a key dst lacks goes to dst's overflow row (or is dropped:
                    // mergeDataOnlyExistingKeysImpl)
                    if (t.ovf)
                        merge_tuple_words(LdsRowSink{s_ovf}, ws, rehash, src_words, src_stride, i);
                }
                else
                    merge_tuple_words(GlobalSink(t, slot), ws, rehash, src_words, src_stride, i);
            }
        }
        const u64 b = __ballot(failed);
        if (pending && lane == 0)
            pending[g] = b;
        if (b != 0 && lane == 0)
            t.ctrl->overflow = 1;
    }
    if (!soft_limit)
    {
        u32 tot = my_claims;
#pragma unroll
        for (int dlt = 32; dlt >= 1; dlt >>= 1)
            tot += __shfl_xor(tot, dlt, WAVE);
        if (lane == 0 && tot)
            atomicAdd(&t.ctrl->stripe[agg_stripe()][0], (unsigned long long)tot);
    }
    if (t.ovf)
    {
        __syncthreads();
        ovf_flush(t, s_ovf, ws, nullptr, true, AGG_MERGE_SENTINEL);
    }
}

__global__ __launch_bounds__(256) void k_occupied_mask(const u64 * __restrict__ keys, u64 capacity, const AggCtrl * __restrict__ ctrl, u8 * __restrict__ mask)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i <= capacity; i += (u64)gridDim.x * 256)
        mask[i] = (i == capacity) ? (ctrl->has_zero != 0) : (keys[i] != 0);
}

__global__ __launch_bounds__(256) void k_fix_zero_key(u64 * __restrict__ keys, u64 capacity)
{
    // the zero-key cell's key word is never written by emplace; make it read as 0 for the exported key column
    if (blockIdx.x == 0 && threadIdx.x == 0)
        keys[capacity] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void k_narrow_keys(const u64 * __restrict__ in, u64 n, T * __restrict__ out)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
        out[i] = (T)in[i];
}

// AvgFraction::divide (AggregateFunctionAvg.h:61-67): Float64(numerator) / denominator
__global__ __launch_bounds__(256) void k_avg_divide(const u64 * __restrict__ num, const u64 * __restrict__ den, u64 n, int num_type, double * __restrict__ out)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        double x;
        if (num_type == CHGPU_F64)
            x = __longlong_as_double((long long)num[i]);
        else if (num_type == CHGPU_I64)
            x = (double)(i64)num[i];
        else
            x = (double)num[i];
        out[i] = x / (double)den[i];
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static u64 pow2_ceil(u64 x)
{
    u64 p = 1;
    while (p < x)
        p <<= 1;
    return p;
}

static int agg_alloc_table(chgpu_agg * a, u64 capacity, AggTable * t, void ** mem, size_t * mem_class)
{
    const size_t cells = capacity + 1;
    const size_t bytes = cells * 8 * (1 + a->words.n_words) + AGG_HDR_BYTES;
    void * m = nullptr;
    CHGPU_TRY(chgpu_pool_alloc(a->ctx, bytes, &m, mem_class));
    hipError_t e = hipMemsetAsync(m, 0, bytes, a->ctx->stream); // HashTableAllocator zero-fills (HashTableAllocator.h:11)
    if (e != hipSuccess)
    {
        chgpu_pool_free(a->ctx, m, *mem_class);
        return chgpu_set_error(CHGPU_ERR_DEVICE, "memset: %s", hipGetErrorString(e));
    }
    t->ctrl = (AggCtrl *)m;
    t->keys = (u64 *)((char *)m + AGG_HDR_BYTES);
    t->words = t->keys + cells;
    t->capacity = capacity;
    t->max_fill = capacity / 2;
    *mem = m;
    return CHGPU_OK;
}

static int agg_read_ctrl(chgpu_agg * a, AggCtrl * out)
{
    CHGPU_TRY(chgpu_read_back(a->ctx, a->t.ctrl, out, sizeof(AggCtrl)));
    out->n_groups = 0;
    for (u32 s = 0; s < AGG_STRIPES; ++s)
        out->n_groups += out->stripe[s][0];
    a->n_groups = out->n_groups;
    CHGPU_REQUIRE(!out->fatal, CHGPU_ERR_LOGICAL, "aggregation table filled completely during a flush");
    return CHGPU_OK;
}

// resize (HashTable.h:504-560): new capacity per the reference's grower, rehash every occupied cell
static int agg_grow(chgpu_agg * a, u64 min_groups, bool has_zero)
{
    u64 cap = a->t.capacity;
    do
    {
        // HashTableGrowerWithPrecalculation::increaseSize (HashTable.h:303): degree += degree >= 23 ? 1 : 2
        cap = cap >= (1ull << 23) ? cap * 2 : cap * 4;
    } while (cap / 2 <= min_groups);
    AggTable nt;
    void * nmem = nullptr;
    size_t nclass = 0;
    CHGPU_TRY(agg_alloc_table(a, cap, &nt, &nmem, &nclass));
    // old cells [0, capacity) plus the out-of-line zero cell when it is set; no soft limit: the new table fits them all
    const u64 n = a->t.capacity + (has_zero ? 1 : 0);
    const u32 grid = chgpu_grid_for(a->ctx, n, AGG_THREADS, 8);
    hipLaunchKernelGGL(k_agg_tuples<AGG_MODE_ALL>, dim3(grid), dim3(AGG_THREADS), 0, a->ctx->stream, nt, AggMergeWords(a->words), 1u, a->t.keys, a->t.words,
                       a->t.capacity + 1, n, 1, has_zero ? a->t.capacity : ~0ull, 0, (u64 *)nullptr);
    a->ctx->counters[6] += 1;
    a->ctx->counters[7] += 1;
    CHGPU_HIP(hipGetLastError());
    chgpu_pool_free(a->ctx, a->table_mem, a->table_class); // stream-ordered: later users queue behind the rehash
    a->table_mem = nmem;
    a->table_class = nclass;
    a->t = nt;
    return CHGPU_OK;
}

// size_hint: the groups promised for the rows of the call that makes the table.
// min_cells: what the first strategy to touch the table wants it to hold (the partitioned path's flush slack): a table that
// does not exist yet is created that large at once instead of being created small and rehashed empty a moment later
static int agg_ensure_table(chgpu_agg * a, u64 size_hint, u64 min_cells = 0)
{
    if (a->table_mem)
        return CHGPU_OK;
    u64 cap = pow2_ceil(size_hint * 2);
    if (cap < AGG_MIN_CAPACITY)
        cap = AGG_MIN_CAPACITY;
    if (cap < min_cells)
        cap = pow2_ceil(min_cells);
    return agg_alloc_table(a, cap, &a->t, &a->table_mem, &a->table_class);
}

// find-only mode leaves the table as it is, so nothing else resets the flag a pending row raised (a grown table starts with a clean header)
static int agg_clear_overflow_flag(chgpu_agg * a)
{
    CHGPU_HIP(hipMemsetAsync(&a->t.ctrl->overflow, 0, sizeof(u32), a->ctx->stream));
    return CHGPU_OK;
}

// The overflow row's words exist from the first call after overflow_row was turned on (zero states: an aggregation without key that saw
// no row).  Kept out of the table: exports, finalize and chgpu_agg_size never see it; the rehash leaves it where it is.
static int agg_ensure_overflow_row(chgpu_agg * a)
{
    if (!a->overflow_row || a->key_type < 0 || a->ovf_mem)
        return CHGPU_OK;
    CHGPU_TRY(chgpu_pool_alloc(a->ctx, AGG_MAX_WORDS * 8, &a->ovf_mem, &a->ovf_class));
    CHGPU_HIP(hipMemsetAsync(a->ovf_mem, 0, AGG_MAX_WORDS * 8, a->ctx->stream));
    return CHGPU_OK;
}

// Enters / leaves find-only mode for the launches of one call (executeOnBlock with no_more_keys, a find-only merge step)
static void agg_set_find_only(chgpu_agg * a, bool on)
{
    a->t.find_only = on ? 1u : 0u;
    a->t.ovf = on ? (u64 *)a->ovf_mem : nullptr;
}

// The state words of every function, from kinds / arg_types / val_types / cond_modes: word_off, the word masks, the `seen` words of
// the conditioned functions and the appended high halves of the fixed-point sums.  Over AGG_MAX_WORDS words: `too_many` and a message.
static int agg_layout(chgpu_agg * a, int too_many)
{
    AggWords & ws = a->words;
    ws = AggWords{};
    a->has_extremum = false;
    u32 w = 0;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        if (w >= AGG_MAX_WORDS)
            return chgpu_set_error(too_many, "more than %u state words: CPU path", AGG_MAX_WORDS);
        const int kind = a->kinds[j];
        const AggKind & k = agg_kind(kind);
        a->word_off[j] = w;
        a->has_extremum = a->has_extremum || k.extremum;
        if (k.words == 3) // {val key, claim, arg}
        {
            if (w + 3 <= AGG_MAX_WORDS)
                ws.arg |= 1u << w;
        }
        else if (k.extremum)
        {
            ws.max |= 1u << w; // order keys, any()'s claim
            if (kind == CHGPU_AGG_ANY)
                ws.any |= 1u << w;
        }
        else if (k.slots && chgpu_type_is_float(a->arg_types[j]))
            ws.f64 |= 1u << w;
        w += k.words;
        // the `seen` word: a zeroed min / max word is also the state of a row that holds the type's extremum, and a NULL-mode sum of 0
        // is not NULL (avg has its denominator, count itself, any / argMin / argMax their claim)
        const bool seen = a->cond_modes[j] != CHGPU_AGG_COND_NONE &&
                          (kind == CHGPU_AGG_MIN || kind == CHGPU_AGG_MAX || (kind == CHGPU_AGG_SUM && a->cond_modes[j] == CHGPU_AGG_COND_NULL));
        if (seen)
        {
            if (w < AGG_MAX_WORDS)
                ws.seen |= 1u << w;
            ++w;
        }
    }
    if (w > AGG_MAX_WORDS)
        return chgpu_set_error(too_many, "more than %u state words: CPU path", AGG_MAX_WORDS);
    ws.n_pub_words = w;
    if (a->key_type >= 0 && chgpu_opt(a->ctx, "deterministic_float_sums", 1))
    {
        // (every Float64 word so far is a function's first: a sum or an avg numerator)
        if (w + (u32)__builtin_popcount(ws.f64) <= AGG_MAX_WORDS) // (more words than the masks hold: such an aggregation keeps its double states)
            for (u32 j = 0; j < a->n_aggs; ++j)
            {
                const u32 lo = a->word_off[j];
                if (ws.op(lo) != 1)
                    continue;
                ws.f64 &= ~(1u << lo); // the low half combines by an integer add
                ws.fx |= 1u << lo;
                ws.fx_high |= 1u << w;
                ws.fx_hi[lo] = (unsigned char)w;
                ++w;
            }
    }
    ws.n_words = w;
    return CHGPU_OK;
}

extern "C" int chgpu_agg_create(chgpu_ctx * ctx, int key_type, uint32_t n_aggs, const int * agg_kinds, const int * arg_types,
                                uint64_t size_hint, chgpu_agg ** out)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(ctx && out && (agg_kinds || n_aggs == 0), CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(n_aggs <= AGG_MAX_AGGS, CHGPU_ERR_NOT_IMPLEMENTED, "more than %u aggregate functions: CPU path", AGG_MAX_AGGS);
    CHGPU_REQUIRE(key_type < 0 || (chgpu_type_is_int(key_type)),
                  CHGPU_ERR_NOT_IMPLEMENTED, "GROUP BY key type %d: CPU path", key_type);
    chgpu_agg * a = new chgpu_agg();
    a->ctx = ctx;
    a->key_type = key_type;
    a->n_aggs = n_aggs;
    a->size_hint = size_hint;
    u32 slot = 0;
    for (u32 j = 0; j < n_aggs; ++j)
    {
        const int kind = agg_kinds[j];
        if (!agg_kind_known(kind))
        {
            delete a;
            return chgpu_set_error(CHGPU_ERR_NOT_IMPLEMENTED, "aggregate function kind %d has no device state: CPU path", kind);
        }
        const u32 n_args = agg_kind(kind).slots; // (two: arg, then val)
        const int at = (n_args == 0 || !arg_types) ? CHGPU_U64 : arg_types[slot];
        const int vt = (n_args == 2 && arg_types) ? arg_types[slot + 1] : CHGPU_U64;
        if (n_args && (!chgpu_type_size(at) || !chgpu_type_size(vt)))
        {
            delete a;
            return chgpu_set_error(CHGPU_ERR_BAD_ARGUMENTS, "bad argument type %d", chgpu_type_size(at) ? vt : at);
        }
        a->kinds[j] = kind;
        a->arg_types[j] = at;
        a->val_types[j] = vt;
        a->slot[j] = slot;
        slot += n_args ? n_args : 1; // (count() keeps its place in arg_cols: without the two-argument kinds slot j is aggregate j)
    }
    a->n_slots = slot;
    const int rc = agg_layout(a, CHGPU_ERR_NOT_IMPLEMENTED);
    if (rc != CHGPU_OK)
    {
        delete a;
        return rc;
    }
    memset(a->host_words, 0, sizeof(a->host_words));
    chgpu_ctx_retain(ctx);
    *out = a;
    return CHGPU_OK;
}

extern "C" int chgpu_agg_set_conditions(chgpu_agg * a, const int * cond_modes)
{
    CHGPU_REQUIRE(a && cond_modes, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(!a->started, CHGPU_ERR_BAD_ARGUMENTS, "aggregate conditions must be set before the first block or merge");
    bool any = false;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        CHGPU_REQUIRE(cond_modes[j] >= CHGPU_AGG_COND_NONE && cond_modes[j] <= CHGPU_AGG_COND_NULL, CHGPU_ERR_BAD_ARGUMENTS, "unknown condition mode %d of function %u",
                      cond_modes[j], j);
        any = any || cond_modes[j] != CHGPU_AGG_COND_NONE;
    }
    int before[AGG_MAX_AGGS];
    memcpy(before, a->cond_modes, sizeof(before));
    const bool was = a->conditioned;
    for (u32 j = 0; j < a->n_aggs; ++j)
        a->cond_modes[j] = cond_modes[j];
    a->conditioned = any;
    const int rc = agg_layout(a, CHGPU_ERR_BAD_ARGUMENTS);
    if (rc != CHGPU_OK)
    {
        // (the message is set; the aggregator keeps the layout it had)
        memcpy(a->cond_modes, before, sizeof(before));
        a->conditioned = was;
        (void)agg_layout(a, CHGPU_ERR_BAD_ARGUMENTS);
        return chgpu_set_error(CHGPU_ERR_BAD_ARGUMENTS, "aggregate conditions need more than %u state words: CPU path", AGG_MAX_WORDS);
    }
    return CHGPU_OK;
}

extern "C" int chgpu_agg_free(chgpu_agg * a)
{
    ChgpuDeviceGuard _dev_guard(a ? a->ctx : nullptr);
    if (!a)
        return CHGPU_OK;
    if (a->table_mem)
        chgpu_pool_free(a->ctx, a->table_mem, a->table_class);
    if (a->ovf_mem)
        chgpu_pool_free(a->ctx, a->ovf_mem, a->ovf_class);
    chgpu_ctx * ctx = a->ctx;
    delete a;
    chgpu_ctx_release(ctx);
    return CHGPU_OK;
}

// The slots of function j in arg_cols: [a->slot[j], agg_slot_end(a, j)) -- none for count()
static u32 agg_slot_end(const chgpu_agg * a, u32 j) { return a->slot[j] + agg_kind(a->kinds[j]).slots; }

// Numbers the distinct condition columns of the block being added (a column shared by several functions is read, filtered or turned
// into a mask once): of[j] = the number of conditioned function j's column, first[c] = the first function that carries column c.
// by_mode: functions share a number only when their modes agree too (without key: one mask per column and mode).  Returns the count.
// A column is told by its data pointer: two column objects over the same bytes count as one (the filtered copy and the without-key
// mask used to tell them by object and made one each; the result is the same, they hold the same bytes).
static u32 agg_number_conds(const chgpu_agg * a, bool by_mode, u32 * of, u32 * first)
{
    u32 n = 0;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        if (a->cond_modes[j] == CHGPU_AGG_COND_NONE)
            continue;
        u32 c = 0;
        while (c < n && !(a->block_conds[first[c]]->data == a->block_conds[j]->data && (!by_mode || a->cond_modes[first[c]] == a->cond_modes[j])))
            ++c;
        if (c == n)
            first[n++] = j;
        of[j] = c;
    }
    return n;
}

static void agg_fill_desc(const chgpu_agg * a, const chgpu_col * const * arg_cols, AggDesc * d)
{
    d->n_aggs = a->n_aggs;
    d->words = a->words;
    d->fx_base = a->fx_base;
    d->row_seq = 0;
    d->arg_sentinel = 0;
    for (u32 w = 0; w < AGG_MAX_WORDS; ++w)
        d->word_map[w] = (unsigned char)w;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        const u32 sl = a->slot[j];
        d->a[j].ptr = (arg_cols && arg_cols[sl]) ? arg_cols[sl]->data : nullptr;
        d->a[j].val = (agg_kind(a->kinds[j]).slots == 2 && arg_cols && arg_cols[sl + 1]) ? arg_cols[sl + 1]->data : nullptr;
        d->a[j].kind = a->kinds[j];
        d->a[j].arg_type = a->arg_types[j];
        d->a[j].val_type = a->val_types[j];
        d->a[j].word = a->word_off[j];
        d->a[j].pre = 0;
        d->a[j].cond = -1;
        d->a[j].cond_want = 0;
        d->a[j].seen = 0;
    }
    d->n_conds = 0;
    for (u32 j = 0; j < AGG_MAX_AGGS; ++j)
        d->cond[j] = nullptr;
    if (!a->conditioned || !a->block_conds)
        return;
    u32 cond_of[AGG_MAX_AGGS], first[AGG_MAX_AGGS];
    d->n_conds = agg_number_conds(a, false, cond_of, first);
    for (u32 c = 0; c < d->n_conds; ++c)
        d->cond[c] = (const u8 *)a->block_conds[first[c]]->data;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        if (a->cond_modes[j] == CHGPU_AGG_COND_NONE)
            continue;
        d->a[j].cond = (signed char)cond_of[j];
        d->a[j].cond_want = a->cond_modes[j] == CHGPU_AGG_COND_IF ? 1 : 0;
        d->a[j].seen = (unsigned char)((a->words.seen >> (a->word_off[j] + agg_kind(a->kinds[j]).words)) & 1);
    }
}

// min / max / any WITHOUT key (executeWithoutKeyImpl, Aggregator.cpp:1276-1321: addBatchSinglePlace): one order-key maximum over the rows of
// the block that pass `cond`; the first such row for any()
__global__ __launch_bounds__(256) void k_nokey_extremum(const void * __restrict__ p, int type, u64 row_begin, u64 n, const u8 * __restrict__ cond, int is_min,
                                                         int val_key, unsigned long long * __restrict__ out)
{
    u64 best = 0;
    for (u64 r = (u64)blockIdx.x * 256 + threadIdx.x; r < n; r += (u64)gridDim.x * 256)
    {
        const u64 i = row_begin + r;
        if (cond && !cond[i])
            continue;
        const u64 bits = load_arg_bits(p, type, i);
        const u64 k = val_key ? agg_val_key(bits, type) : agg_order_key(bits, type);
        const u64 v = is_min ? ~k : k;
        best = v > best ? v : best;
    }
#pragma unroll
    for (int dlt = 32; dlt >= 1; dlt >>= 1)
    {
        const u64 o = ((u64)(u32)__shfl_xor((int)(u32)(best >> 32), dlt, WAVE) << 32) | (u32)__shfl_xor((int)(u32)best, dlt, WAVE);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0 && best)
        atomicMax(out, (unsigned long long)best);
}
__global__ __launch_bounds__(256) void k_nokey_first_row(u64 row_begin, u64 n, const u8 * __restrict__ cond, unsigned long long * __restrict__ out)
{
    u64 first = ~0ull;
    for (u64 r = (u64)blockIdx.x * 256 + threadIdx.x; r < n && first == ~0ull; r += (u64)gridDim.x * 256)
        if (!cond || cond[row_begin + r])
            first = r;
    if (first != ~0ull)
        atomicMin(out, (unsigned long long)first);
}
// argMin / argMax without key: the first row of the block that passes `cond` and holds the val key `want` (k_nokey_extremum's result)
__global__ __launch_bounds__(256) void k_nokey_first_holder(const void * __restrict__ p, int type, u64 row_begin, u64 n, const u8 * __restrict__ cond, int is_min,
                                                             u64 want, unsigned long long * __restrict__ out)
{
    u64 first = ~0ull;
    for (u64 r = (u64)blockIdx.x * 256 + threadIdx.x; r < n && first == ~0ull; r += (u64)gridDim.x * 256)
    {
        const u64 i = row_begin + r;
        if (cond && !cond[i])
            continue;
        const u64 k = agg_val_key(load_arg_bits(p, type, i), type);
        if ((is_min ? ~k : k) == want)
            first = r;
    }
    if (first != ~0ull)
        atomicMin(out, (unsigned long long)first);
}
__global__ void k_nokey_load(const void * __restrict__ p, int type, u64 i, u64 * __restrict__ out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0)
        out[0] = load_arg_bits(p, type, i);
}

// any(): the second pass of a block.  Every group's claim word now names the earliest of its rows (all blocks so far); the row a claim
// names stores its value.  Claims set by earlier blocks name rows of those blocks: no row of this block matches them, the value stays.
__global__ __launch_bounds__(AGG_THREADS) void k_agg_any_resolve(AggTable t, AggDesc d, const void * __restrict__ keys, int key_type, u64 row_begin, u64 n)
{
    const u64 stride = t.capacity + 1, mask = t.capacity - 1;
    for (u64 r = (u64)blockIdx.x * AGG_THREADS + threadIdx.x; r < n; r += (u64)gridDim.x * AGG_THREADS)
    {
        const u64 i = row_begin + r;
        const u64 key = load_key_zext(keys, key_type, i);
        const u32 nz = cond_row_bits(d, i); // (a claim only ever came from a row that reached the function: the test saves the state's load)
        u64 slot = t.capacity; // the zero key's cell
        if (t.find_only)
        {
            // a find-only block: the table is as the rows saw it, so a row that missed it missed it here too and claimed the overflow row
            slot = table_find(t, key);
            if (slot == AGG_SLOT_MISS)
            {
                if (t.ovf)
                    for (u32 j = 0; j < d.n_aggs; ++j)
                        if (d.a[j].kind == CHGPU_AGG_ANY && cond_reaches(d.a[j], nz) && t.ovf[d.a[j].word] == ~(d.row_seq + i))
                            t.ovf[d.a[j].word + 1] = load_arg_bits(d.a[j].ptr, d.a[j].arg_type, i);
                continue;
            }
        }
        else if (key != 0)
        {
            slot = dev_intHash64(key) & mask;
            for (u64 step = 0; step < t.capacity; ++step)
            {
                const u64 k = t.keys[slot];
                if (k == key || k == 0)
                    break;
                slot = (slot + 1) & mask;
            }
            if (t.keys[slot] != key)
                continue; // (every row of the block was placed before this pass: not reached)
        }
        const u64 claim = ~(d.row_seq + i);
        for (u32 j = 0; j < d.n_aggs; ++j)
            if (d.a[j].kind == CHGPU_AGG_ANY && cond_reaches(d.a[j], nz) && t.words[(u64)d.a[j].word * stride + slot] == claim)
                t.words[(u64)(d.a[j].word + 1) * stride + slot] = load_arg_bits(d.a[j].ptr, d.a[j].arg_type, i);
    }
}

// ---- argMin / argMax: the claim and resolve passes ----
// "The earliest row among those that hold the extremum" cannot be folded in one atomic: a group's extremum is only known once every row
// of the block has been seen.  The block pass (add_row) raised every val key; after that kernel boundary the val keys are final for the
// block, and PASS 2 lets every row whose key EQUALS its group's claim with agg_arg_row_claim(ordinal) under an unsigned max; after the
// next boundary the claims are final and PASS 3 lets the row a claim names store its arg.  A claim of an earlier block (or of a merge, ~0) beats every
// row of this block, so a row that only equals the extremum changes nothing; a raised extremum starts from the block's sentinel, which
// every row of the block beats.
// The state of `key` as the block pass left it: its cell, or in a find-only block the overflow row for a key the table lacks (no state
// when there is no overflow row: the row was dropped).  base[w * stride] is table word w.
__device__ __forceinline__ bool agg_state_of(const AggTable & t, u64 key, u64 *& base, u64 & stride)
{
    const u64 slot = table_find(t, key);
    if (slot == AGG_SLOT_MISS)
    {
        if (!t.find_only || !t.ovf)
            return false; // (not find-only: every row of the block was placed before this pass, not reached)
        base = t.ovf;
        stride = 1;
        return true;
    }
    base = t.words + slot;
    stride = t.capacity + 1;
    return true;
}
// PASS 2: `claim` under an unsigned max when the state's val key is `key`; PASS 3: the state's arg from `arg_bits` when its claim is
// `claim`, and the claim itself replaced by `settled` when that is non-zero (merges: ~0).  st = the state's val key word.
template <int PASS>
__device__ __forceinline__ void agg_arg_claim_or_resolve(u64 * st, u64 stride, u64 key, u64 claim, u64 arg_bits, u64 settled)
{
    if (*st != key)
        return;
    unsigned long long * c = (unsigned long long *)(st + stride);
    if (PASS == 2)
    {
        // (the load keeps a group of equal rows from queueing on one address: most of them see a claim above their own)
        if (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < claim)
            __hip_atomic_fetch_max(c, (unsigned long long)claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    else if (*c == claim)
    {
        st[2 * stride] = arg_bits;
        if (settled)
            *c = settled; // only the winner writes, and no other claim of this pass equals either value
    }
}
template <int PASS>
__global__ __launch_bounds__(AGG_THREADS) void k_agg_arg_rows(AggTable t, AggDesc d, const void * __restrict__ keys, int key_type, u64 row_begin, u64 n)
{
    for (u64 r = (u64)blockIdx.x * AGG_THREADS + threadIdx.x; r < n; r += (u64)gridDim.x * AGG_THREADS)
    {
        const u64 i = row_begin + r;
        u64 * base;
        u64 stride;
        if (!agg_state_of(t, load_key_zext(keys, key_type, i), base, stride))
            continue;
        const u32 nz = cond_row_bits(d, i);
        for (u32 j = 0; j < d.n_aggs; ++j)
        {
            const AggArg & a = d.a[j];
            if (a.kind != CHGPU_AGG_ARG_MIN && a.kind != CHGPU_AGG_ARG_MAX)
                continue;
            if (!cond_reaches(a, nz))
                continue; // a masked-out row may EQUAL the extremum: it must not claim it
            const u64 k = agg_val_key(load_arg_bits(a.val, a.val_type, i), a.val_type);
            agg_arg_claim_or_resolve<PASS>(base + (u64)a.word * stride, stride, a.kind == CHGPU_AGG_ARG_MAX ? k : ~k, agg_arg_row_claim(d.row_seq + i),
                                           PASS == 3 ? load_arg_bits(a.ptr, a.arg_type, i) : 0, 0);
        }
    }
}
// The same two passes of a merge, over the source tuples k_agg_tuples folded in: tuple i claims with AGG_MERGE_CLAIM_TOP - i.
template <int PASS>
__global__ __launch_bounds__(AGG_THREADS) void k_agg_arg_tuples(AggTable t, AggWords ws, const u64 * __restrict__ src_keys,
                                                                const u64 * __restrict__ src_words, u64 src_stride, u64 n, int skip_zero_keys, u64 zero_slot_index)
{
    for (u64 i = (u64)blockIdx.x * AGG_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * AGG_THREADS)
    {
        u64 key = src_keys[i];
        const bool is_zero_cell = (i == zero_slot_index);
        if (is_zero_cell)
            key = 0;
        if (skip_zero_keys && key == 0 && !is_zero_cell)
            continue;
        u64 * base;
        u64 stride;
        if (!agg_state_of(t, key, base, stride))
            continue;
        for (u32 w = 0; w + 2 < ws.n_words; ++w)
            if (((ws.arg >> w) & 1) && src_words[(u64)(w + 1) * src_stride + i] != 0)
                agg_arg_claim_or_resolve<PASS>(base + (u64)w * stride, stride, src_words[(u64)w * src_stride + i], AGG_MERGE_CLAIM_TOP - i,
                                               src_words[(u64)(w + 2) * src_stride + i], ~0ull);
    }
}

// ---- the fixed-point window of the deterministic Float64 sums (see Fx128) ----
// Over the non-zero finite values (as doubles; a subnormal counts as exponent 1): out[0] = largest biased exponent (0 = no such value),
// out[2] = 2047 - smallest biased exponent; out[1] = 1 when some value is NaN / +-inf.  cond (may be NULL): only the rows whose byte
// is non-zero (cond_want 1) / zero (cond_want 0) are looked at -- a value the function never sees must not shape its window.
__global__ __launch_bounds__(256) void k_fx_exp_stats(const void * __restrict__ p, int type, u64 row_begin, u64 n, const u8 * __restrict__ cond, int cond_want,
                                                       u32 * __restrict__ out)
{
    u32 emax = 0, emin_c = 0, bad = 0;
    auto take = [&](u64 bits) {
        u32 e = (u32)(bits >> 52) & 0x7ffu;
        if (e == 0x7ffu)
            bad = 1;
        else if (bits << 1)
        {
            e = e ? e : 1u;
            emax = e > emax ? e : emax;
            emin_c = 2047u - e > emin_c ? 2047u - e : emin_c;
        }
    };
    const u64 tid = (u64)blockIdx.x * 256 + threadIdx.x, nthreads = (u64)gridDim.x * 256;
    if (cond)
    {
        for (u64 i = tid; i < n; i += nthreads)
            if ((int)(__builtin_nontemporal_load(cond + row_begin + i) != 0) == cond_want)
                take(load_arg_bits(p, type, row_begin + i));
    }
    else if (type == CHGPU_F64 && (((uintptr_t)p + row_begin * 8) & 15) == 0)
    {
        // a streaming read: two 16-byte nontemporal loads per lane in flight
        typedef u64 v2q __attribute__((ext_vector_type(2)));
        const v2q * q = (const v2q *)((const u64 *)p + row_begin);
        const u64 pairs = n / 2;
        u64 i = tid;
        for (; i + nthreads < pairs; i += 2 * nthreads)
        {
            const v2q a = __builtin_nontemporal_load(q + i), b = __builtin_nontemporal_load(q + i + nthreads);
            take(a.x), take(a.y), take(b.x), take(b.y);
        }
        for (; i < pairs; i += nthreads)
        {
            const v2q a = __builtin_nontemporal_load(q + i);
            take(a.x), take(a.y);
        }
        if ((n & 1) && tid == 0)
            take(((const u64 *)p)[row_begin + n - 1]);
    }
    else
        for (u64 i = tid; i < n; i += nthreads)
            take(load_arg_bits(p, type, row_begin + i));
#pragma unroll
    for (int dlt = 32; dlt >= 1; dlt >>= 1)
    {
        const u32 o = (u32)__shfl_xor((int)emax, dlt, WAVE), q2 = (u32)__shfl_xor((int)emin_c, dlt, WAVE);
        emax = o > emax ? o : emax;
        emin_c = q2 > emin_c ? q2 : emin_c;
    }
    const u64 anybad = __ballot(bad != 0);
    if ((threadIdx.x & 63) == 0)
    {
        if (emax)
        {
            atomicMax(&out[0], emax);
            atomicMax(&out[2], emin_c);
        }
        if (anybad)
            out[1] = 1;
    }
}
// every state of one pair shifted right by sh bits (arithmetic: floor), the window's unit growing from 2^base to 2^(base + sh)
__global__ __launch_bounds__(256) void k_fx_shift(u64 * __restrict__ lo, u64 * __restrict__ hi, u64 cells, int sh)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < cells; i += (u64)gridDim.x * 256)
    {
        const u64 l = lo[i], h = hi[i];
        if ((l | h) == 0)
            continue;
        u64 nl, nh;
        if (sh >= 128)
            nl = nh = (u64)((i64)h >> 63);
        else if (sh >= 64)
            nl = (u64)((i64)h >> (sh - 64 < 63 ? sh - 64 : 63)), nh = (u64)((i64)h >> 63);
        else
            nl = (l >> sh) | (h << (64 - sh)), nh = (u64)((i64)h >> sh);
        lo[i] = nl;
        hi[i] = nh;
    }
}
// out[i] = the pair as a double (out may be lo itself); hi is cleared when clear_hi
__global__ __launch_bounds__(256) void k_fx_to_double(u64 * __restrict__ lo, u64 * __restrict__ hi, u64 n, int base, int clear_hi)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const double v = fx_to_double(lo[i], hi[i], base);
        lo[i] = (u64)__double_as_longlong(v);
        if (clear_hi)
            hi[i] = 0;
    }
}
__global__ __launch_bounds__(256) void k_fx_from_double(const u64 * __restrict__ src, u64 n, int base, u64 * __restrict__ lo, u64 * __restrict__ hi)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const Fx128 x = fx_from_double(src[i], base);
        lo[i] = x.lo;
        hi[i] = x.hi;
    }
}

static int agg_fx_shift(chgpu_agg * a, int sh)
{
    if (sh <= 0)
        return CHGPU_OK;
    const u64 cells = a->t.capacity + 1;
    for (u32 w = 0; w < a->words.n_pub_words; ++w)
        if ((a->words.fx >> w) & 1)
        {
            if (a->table_mem)
            {
                hipLaunchKernelGGL(k_fx_shift, dim3(chgpu_grid_for(a->ctx, cells, 256, 8)), dim3(256), 0, a->ctx->stream, a->t.words + (u64)w * cells,
                                   a->t.words + (u64)a->words.fx_hi[w] * cells, cells, sh);
                a->ctx->counters[6] += 1;
            }
            if (a->ovf_mem) // the overflow row's pair moves with the window too (it may exist before the table: is_overflows blocks)
            {
                hipLaunchKernelGGL(k_fx_shift, dim3(1), dim3(256), 0, a->ctx->stream, (u64 *)a->ovf_mem + w, (u64 *)a->ovf_mem + a->words.fx_hi[w], (u64)1, sh);
                a->ctx->counters[6] += 1;
            }
        }
    CHGPU_HIP(hipGetLastError());
    return CHGPU_OK;
}
// Moves the window to (base, log_cap); never narrows it.
static int agg_fx_set_window(chgpu_agg * a, int base, int log_cap)
{
    if (!a->fx_base_set)
    {
        a->fx_base = base;
        a->fx_log_cap = log_cap;
        a->fx_base_set = true;
        return CHGPU_OK;
    }
    if (base > a->fx_base)
        CHGPU_TRY(agg_fx_shift(a, base - a->fx_base));
    a->fx_base = base > a->fx_base ? base : a->fx_base;
    a->fx_log_cap = log_cap > a->fx_log_cap ? log_cap : a->fx_log_cap;
    return CHGPU_OK;
}
// The aggregation goes back to double states (a NaN or an infinity cannot be a fixed-point value: from here on its sums behave like the
// reference's, poisoned groups included); every pair becomes the double it stands for.
static int agg_fx_to_plain(chgpu_agg * a)
{
    if (!a->words.fx)
        return CHGPU_OK;
    const u64 cells = a->t.capacity + 1;
    for (u32 w = 0; w < a->words.n_pub_words; ++w)
        if ((a->words.fx >> w) & 1)
        {
            if (a->table_mem)
            {
                hipLaunchKernelGGL(k_fx_to_double, dim3(chgpu_grid_for(a->ctx, cells, 256, 8)), dim3(256), 0, a->ctx->stream, a->t.words + (u64)w * cells,
                                   a->t.words + (u64)a->words.fx_hi[w] * cells, cells, a->fx_base, 1);
                a->ctx->counters[6] += 1;
            }
            if (a->ovf_mem) // (with or without a table)
            {
                hipLaunchKernelGGL(k_fx_to_double, dim3(1), dim3(256), 0, a->ctx->stream, (u64 *)a->ovf_mem + w, (u64 *)a->ovf_mem + a->words.fx_hi[w], (u64)1,
                                   a->fx_base, 1);
                a->ctx->counters[6] += 1;
            }
        }
    CHGPU_HIP(hipGetLastError());
    a->words.f64 |= a->words.fx;
    a->words.fx = 0; // (fx_high stays: the spare words keep being skipped; they hold zeros)
    return CHGPU_OK;
}
// exponent statistics of `n` values of one column: *emax_biased = 0 when every value is zero (then *emin_biased is 2047)
static int agg_fx_stats(chgpu_ctx * ctx, const void * data, int type, u64 row_begin, u64 n, const u8 * cond, int cond_want, u32 * emax_biased, u32 * emin_biased,
                        bool * nonfinite)
{
    void * scratch = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, 256, &scratch));
    CHGPU_HIP(hipMemsetAsync(scratch, 0, 16, ctx->stream));
    hipLaunchKernelGGL(k_fx_exp_stats, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, data, type, row_begin, n, cond, cond_want, (u32 *)scratch);
    ctx->counters[6] += 1;
    CHGPU_HIP(hipGetLastError());
    u32 r[4];
    CHGPU_TRY(chgpu_read_back(ctx, scratch, r, 16));
    *emax_biased = r[0];
    *emin_biased = 2047u - r[2];
    *nonfinite = r[1] != 0;
    return CHGPU_OK;
}
// Every value must keep at least this many significant bits in the window; an input whose magnitudes spread further (2^(97 - 24) = 1e22
// between the largest and the smallest non-zero value, less 8 bits per widening for more than 2^30 rows) goes back to double states.
static constexpr int FX_MIN_BITS = 24;
// Makes room for `n` more values whose biased exponents span [emin, emax] (emax 0 = all of them zero).
static int agg_fx_admit(chgpu_agg * a, u32 emax_biased, u32 emin_biased, u64 n)
{
    if (emax_biased == 0)
    {
        a->fx_rows += n; // zeros fit any window
        return CHGPU_OK;
    }
    int log_cap = a->fx_base_set ? a->fx_log_cap : 30;
    const u64 rows = a->fx_rows + n;
    while (log_cap < 62 && rows > (1ull << log_cap))
        log_cap += 8;
    const int e_unb = (int)emax_biased - 1023;                        // every |x| < 2^(e_unb + 1)
    int base = e_unb + 1 - 127 + log_cap;                             // ... = 2^(127 - log_cap) units
    if (a->fx_base_set && a->fx_base + (log_cap - a->fx_log_cap) > base)
        base = a->fx_base + (log_cap - a->fx_log_cap);                // the states already there keep the invariant
    const int emin = (int)emin_biased - 1023 < a->fx_emin ? (int)emin_biased - 1023 : a->fx_emin;
    if (emin + 1 - FX_MIN_BITS < base) // the smallest value ever added would keep fewer than FX_MIN_BITS bits
        return agg_fx_to_plain(a);
    CHGPU_TRY(agg_fx_set_window(a, base, log_cap));
    a->fx_emin = emin;
    a->fx_rows = rows;
    return CHGPU_OK;
}
// before a block's rows are added: look at the float arguments of the fixed-point sums
static int agg_fx_prepare_block(chgpu_agg * a, const chgpu_col * const * arg_cols, u64 row_begin, u64 n)
{
    if (!a->words.fx || n == 0)
        return CHGPU_OK;
    u32 emax = 0, emin = 2047;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        if (a->kinds[j] == CHGPU_AGG_COUNT || !((a->words.fx >> a->word_off[j]) & 1))
            continue;
        u32 e = 0, em = 2047;
        bool bad = false;
        const chgpu_col * cc = a->cond_modes[j] != CHGPU_AGG_COND_NONE ? a->block_conds[j] : nullptr;
        CHGPU_TRY(agg_fx_stats(a->ctx, arg_cols[a->slot[j]]->data, a->arg_types[j], row_begin, n, cc ? (const u8 *)cc->data : nullptr,
                               a->cond_modes[j] == CHGPU_AGG_COND_IF ? 1 : 0, &e, &em, &bad));
        if (bad)
            return agg_fx_to_plain(a);
        emax = e > emax ? e : emax;
        emin = em < emin ? em : emin;
    }
    return agg_fx_admit(a, emax, emin, n);
}

// ---------------------------------------------------------------------------------------------
// GROUP BY host plans.  Each plan is DECIDED into a plain struct by a function that makes no HIP call (OK, or NOT_IMPLEMENTED = the
// shape does not fit), its scratch is LAID OUT by one carving function, and its kernels are LAUNCHED by a run function that reads
// both.  Between deciding the partition geometry and testing the tile-sorted fit the table is sized (agg_partition_size_table).
// ---------------------------------------------------------------------------------------------

// What a plan is told about its rows besides the columns: the key and argument types as the columns hold them and the groups promised
// for them.  The aggregator's own for a caller's block; a level-2 call of the two-level plan reads partition buffers (4/8-byte keys,
// arguments widened to 8 bytes) and gets its share of the promise.
struct AggInput
{
    int key_type;
    int arg_types[AGG_MAX_AGGS];
    u64 size_hint;
};

static AggInput agg_input_of(const chgpu_agg * a)
{
    AggInput in;
    in.key_type = a->key_type;
    memcpy(in.arg_types, a->arg_types, sizeof(in.arg_types));
    in.size_hint = a->size_hint;
    return in;
}

// Raise the kernel's dynamic LDS limit to `lds_bytes` and launch it (the attribute is set before every launch).  A failure sets the
// error message and clears the sticky launch error, so that it does not surface in the next call.
template <typename Kern, typename... Args>
static int launch_lds(const char * what, Kern kern, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args... args)
{
    hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(kern, grid, block, lds_bytes, stream, args...);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        return CHGPU_OK;
    (void)hipGetLastError();
    return chgpu_set_error(CHGPU_ERR_DEVICE, "%s launch failed: %s", what, hipGetErrorString(e));
}

// Carves one scratch allocation into regions: take<T>(count) gives the next region and advances by its size rounded up to 256 bytes
// (take_packed: by its size as it is); bytes() is the total to ask chgpu_scratch for.  A layout function runs twice over the same
// statements: over a null base for the size, then over the allocation for the pointers.
struct ScratchCarver
{
    uintptr_t base;
    size_t off = 0;
    static size_t al(size_t b) { return (b + 255) / 256 * 256; }
    template <typename T>
    T * take(size_t count)
    {
        T * p = (T *)(base + off);
        off += al(count * sizeof(T));
        return p;
    }
    template <typename T>
    T * take_packed(size_t count)
    {
        T * p = (T *)(base + off);
        off += count * sizeof(T);
        return p;
    }
    size_t bytes() const { return al(off); }
};

// 4-byte (or narrower, stored as 4 bytes) or 8-byte keys of the partition buffers: fn(u32{} / u64{})
template <typename F>
static void dispatch_key(bool key32, F && fn)
{
    if (key32)
        fn(u32{});
    else
        fn(u64{});
}

// Bytes of the compact LDS cell of the partition-aggregate kernel (see PartLds) that holds the state words of the functions in
// `agg_mask`, and which of the aggregator's words are 32-bit counts there: the key as wide as the partition buffers' keys, COUNT words
// as 32 bits while the call has fewer than 2^32 rows.  The full mask is the aggregator's own layout with EVERY word of it: the spare
// high words that fixed-point sums leave behind when they go back to doubles (agg_fx_to_plain) are still there, while a pass over some
// of the functions numbers its words afresh (agg_localise_words) and leaves them out.
static size_t agg_part_cell_bytes(const chgpu_agg * a, int key_type, u64 n, u32 * cnt32_out, u32 agg_mask = ~0u)
{
    const u32 c32 = n < (1ull << 32) && !chgpu_opt(a->ctx, "tune_gb_nocnt32", 0) ? 1 : 0;
    u32 cnt32 = 0, words = 0;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        if (!((agg_mask >> j) & 1))
            continue;
        const u32 w = a->word_off[j];
        words += agg_kind(a->kinds[j]).words + ((a->words.fx >> w) & 1);
        if (a->kinds[j] == CHGPU_AGG_COUNT)
            cnt32 |= c32 << w;
        else if (a->kinds[j] == CHGPU_AGG_AVG)
            cnt32 |= c32 << (w + 1);
    }
    if (agg_mask == ~0u)
        words = a->words.n_words;
    if (cnt32_out)
        *cnt32_out = cnt32;
    const u32 n4 = (u32)__builtin_popcount(cnt32);
    return (chgpu_type_size(key_type) <= 4 ? 4 : 8) + 8 * (words - n4) + 4 * n4;
}

// Largest power-of-two cell count whose table fits ~150 KiB of LDS (at most 8192).
static u32 agg_part_max_cells(const chgpu_ctx * ctx, size_t cell_b)
{
    const u32 s_max = (u32)chgpu_opt(ctx, "tune_gb_s", 8192);
    const u32 s_kib = (u32)chgpu_opt(ctx, "tune_gb_kib", 150);
    u32 S = s_max;
    while ((size_t)(S + 1) * cell_b + 32 > (size_t)s_kib * 1024 && S > 256)
        S >>= 1;
    return S;
}

// Number of distinct keys D that makes a uniform sample of m rows show d distinct ones: d = D (1 - exp(-m / D)).
// (the reference adapts its strategy from observed statistics too: Aggregator.cpp:944-958, :83-89)
static u64 agg_estimate_groups(u64 d, u64 m)
{
    if (d == 0)
        return 0;
    if ((double)d >= 0.97 * (double)m)
        return ~0ull >> 8; // (nearly) every sampled row opened a group: no upper bound can be inferred
    double lo = (double)d, hi = 1e15;
    for (int it = 0; it < 200 && hi / lo > 1.0001; ++it)
    {
        const double mid = std::sqrt(lo * hi);
        const double seen = mid * (1.0 - std::exp(-(double)m / mid));
        if (seen < (double)d)
            lo = mid;
        else
            hi = mid;
    }
    return (u64)hi;
}

// The `debug` option's line for the finish rounds: how many rounds re-ran rows left pending (0: the plan placed every row itself)
static int agg_debug_rounds(const chgpu_ctx * ctx, int rounds)
{
    if (chgpu_opt(ctx, "debug", 0))
        fprintf(stderr, "chgpu: GROUP BY finish rounds=%d\n", rounds);
    return CHGPU_OK;
}

// resize on overflow (HashTable.h:921-944): grow + rehash, then re-run only the rows left pending, until none is.  relaunch(grid):
// the plan's kernel over its n rows that places the rows marked pending.
template <typename Relaunch>
static int agg_finish_rounds_with(chgpu_agg * a, u64 n, Relaunch relaunch)
{
    chgpu_ctx * ctx = a->ctx;
    for (int round = 0; round < 64; ++round)
    {
        AggCtrl c;
        CHGPU_TRY(agg_read_ctrl(a, &c));
        if (!c.overflow && c.n_groups <= a->t.max_fill)
            return agg_debug_rounds(ctx, round);
        if (a->t.find_only)
        {
            // a find-only block never grows the table: the rows a plan left pending are looked up once more (a look-up cannot fail)
            if (!c.overflow)
                return agg_debug_rounds(ctx, round);
            CHGPU_TRY(agg_clear_overflow_flag(a));
        }
        else
        {
            CHGPU_TRY(agg_grow(a, c.n_groups, c.has_zero != 0));
            if (!c.overflow)
                return agg_debug_rounds(ctx, round);
        }
        relaunch(chgpu_grid_for(ctx, n, AGG_THREADS, 8));
        ctx->counters[6] += 1;
        CHGPU_HIP(hipGetLastError());
    }
    return chgpu_set_error(CHGPU_ERR_LOGICAL, "aggregation table did not converge after 64 growth rounds");
}

static int agg_finish_rounds(chgpu_agg * a, const AggDesc & d, const void * keys, int key_type, u64 row_begin, u64 n, u64 * pending)
{
    return agg_finish_rounds_with(a, n, [&](u32 grid) {
        hipLaunchKernelGGL(k_agg_rows_direct<AGG_MODE_PENDING>, dim3(grid), dim3(AGG_THREADS), 0, a->ctx->stream, a->t, d, keys, key_type, row_begin, n, pending);
    });
}

static int agg_finish_rounds_aos(chgpu_agg * a, const AggDesc & d, const u32 * rec, int key64, u64 n, u64 * pending)
{
    return agg_finish_rounds_with(a, n, [&](u32 grid) {
        hipLaunchKernelGGL(k_agg_tiles_pending_aos, dim3(grid), dim3(AGG_THREADS), 0, a->ctx->stream, a->t, d, rec, key64, n, pending);
    });
}

// The descriptor of a pass over a subset of the functions (d->a[0 .. n_aggs) already compacted to them): d->words re-expressed in local
// numbering -- the functions' words 0 .. n-1 in their order (a fixed-point sum's high half behind the regular words, as in the
// aggregator), every per-word mask moved along -- and word_map[] back to the table's words; *cnt32 (which words are 32-bit counts in
// LDS) likewise.
static void agg_localise_words(AggDesc * d, u32 * cnt32)
{
    const AggWords g = d->words;
    const u32 g_cnt32 = *cnt32;
    AggWords l{};
    u32 wl = 0, l_cnt32 = 0;
    u32 fx_lo_local[AGG_MAX_AGGS], n_fx = 0;
    for (u32 m = 0; m < d->n_aggs; ++m)
    {
        const u32 gw = d->a[m].word, words = agg_kind(d->a[m].kind).words;
        d->a[m].word = wl;
        for (u32 x = 0; x < words; ++x)
        {
            d->word_map[wl + x] = (unsigned char)(gw + x);
            l_cnt32 |= ((g_cnt32 >> (gw + x)) & 1u) << (wl + x);
            l.f64 |= ((g.f64 >> (gw + x)) & 1u) << (wl + x);
            l.max |= ((g.max >> (gw + x)) & 1u) << (wl + x);
        }
        if ((g.fx >> gw) & 1)
        {
            l.fx |= 1u << wl;
            fx_lo_local[n_fx++] = wl; // its high half is placed behind the regular words below
        }
        wl += words;
    }
    l.n_pub_words = wl;
    for (u32 k = 0; k < n_fx; ++k, ++wl)
    {
        const u32 lo = fx_lo_local[k];
        d->word_map[wl] = g.fx_hi[d->word_map[lo]];
        l.fx_hi[lo] = (unsigned char)wl;
        l.fx_high |= 1u << wl;
    }
    l.n_words = wl;
    d->words = l;
    *cnt32 = l_cnt32;
}

// The compile-time update code of the state words (OPS of k_agg_part_lds / k_agg_tiles_lds; 7 = a fixed-point Float64 sum, 9 = its
// high word).  0 = no code: more than four words, a word the descriptor leaves untouched, a third argument word (pre >= 2), or a
// fixed-point sum of the second one.
static u32 agg_update_code(const AggDesc & d, u32 cnt32)
{
    if (d.words.n_words > 4)
        return 0;
    u32 word_op[AGG_MAX_WORDS] = {0};
    for (u32 j = 0; j < d.n_aggs; ++j)
    {
        const u32 w = d.a[j].word;
        if (d.a[j].kind == CHGPU_AGG_COUNT)
            word_op[w] = ((cnt32 >> w) & 1) ? 5 : 6;
        else
        {
            if (d.a[j].pre >= 2)
                return 0;
            word_op[w] = (d.a[j].arg_type == CHGPU_F64 ? 3 : 1) + d.a[j].pre;
            if ((d.words.fx >> w) & 1)
            {
                if (d.a[j].pre != 0)
                    return 0;
                word_op[w] = 7, word_op[d.words.fx_hi[w]] = 9;
            }
            if (d.a[j].kind == CHGPU_AGG_AVG)
                word_op[w + 1] = ((cnt32 >> (w + 1)) & 1) ? 5 : 6;
        }
    }
    u32 ops = 0;
    for (u32 w = 0; w < d.words.n_words; ++w)
    {
        if (word_op[w] == 0)
            return 0;
        ops |= word_op[w] << (4 * w);
    }
    return ops;
}

// The update codes each aggregate kernel is instantiated for: the acceptance test of a plan and the switch of its launch read the
// same list.  1 = sum, 3 = sum(Float64), 5 / 6 = a 32- / 64-bit count, 2 = a sum of the second argument word, 97 = a fixed-point pair.
using GbTileOps = OneOf<0x51, 0x15, 0x1, 0x53, 0x3, 0x61, 0x16, 0x97, 0x957, 0x967>; // k_agg_tiles_lds: no other code runs
using GbPartOps = OneOf<0x51, 0x15, 0x1, 0x5, 0x53, 0x3, 0x21, 0x521, 0x97, 0x957>;  // k_agg_part_lds: every other code takes OPS = 0

// Every count() of the aggregation (bit j = function j).  A block that goes over its rows in several passes or calls, each with some
// of the functions, counts in the first of them.
static u32 agg_count_mask(const chgpu_agg * a)
{
    u32 mask = 0;
    for (u32 j = 0; j < a->n_aggs; ++j)
        if (a->kinds[j] == CHGPU_AGG_COUNT)
            mask |= 1u << j;
    return mask;
}

// The functions of `agg_mask` alone in the descriptor (in their order); their state word indices stay the aggregator's own.
static void agg_desc_keep(AggDesc * d, u32 agg_mask)
{
    u32 m = 0;
    for (u32 j = 0; j < d->n_aggs; ++j)
        if ((agg_mask >> j) & 1)
            d->a[m++] = d->a[j];
    d->n_aggs = m;
}

// The partition geometry of one partitioned call, and -- once the scatter plan is the one that runs -- its launch shape.
struct GbPartPlan
{
    int level = 0;       // 0: one level.  1: the first of two (P == P1 big partitions, no aggregate pass).  2: one big partition's call.
    u32 K = 0;           // argument words per row of the partition buffers
    u32 agg_mask = ~0u;  // the functions this call applies
    bool key32 = false;  // keys of <= 4 bytes: 4-byte keys in the partition buffers
    u32 P = 0, P1 = 0;   // partitions of this call; big partitions when level == 1
    u32 S = 0;           // cells of the aggregate pass's LDS table
    u32 cnt32 = 0;       // state words that are 32-bit counts in LDS
    u64 mult = GBP_MULT; // the partition hash's multiplier
    u64 chunk_rows = 0;  // rows per work unit of the aggregate pass
    u64 max_units = 0;   // sum over partitions of ceil(rows_p / chunk_rows), at most
    // the scatter plan (agg_scatter_plan)
    u32 G = 0, tile = 0; // workgroups and tile rows of the partition passes
    u64 rows_per_wg = 0;
    bool wide = false;   // 16-byte loads: columns as wide as the buffers, first row 16-byte aligned
    u32 rp_tile = 0;     // tile of the branch-free scatter (k_rp_scatter) when it runs instead of k_gb_scatter, else 0
    u32 ops = 0;         // update code of the aggregate pass (0: the generic update)
    GbpCols gc;
    AggDesc d;           // argument pointers are set once the partition buffers are laid out
};

// Decides P, S and the work units from the promised groups.  word_pass: a pass over ONE argument word of a subset of the functions
// (level 0, K = 1), which goes through the tile-sorted plan with cells that hold only its words.
static int agg_partition_geometry(const chgpu_agg * a, const AggInput & in, u64 n, u32 K, int level, u32 agg_mask, bool word_pass, GbPartPlan * g)
{
    const chgpu_ctx * ctx = a->ctx;
    g->K = K;
    g->agg_mask = agg_mask;
    // LDS table of the aggregate pass (one 1024-thread workgroup per CU): compact cells -- key as wide as the partition
    // buffer's keys, COUNT words as 32 bits while the call has fewer than 2^32 rows -- and as many cells as fit ~150 KiB
    g->key32 = chgpu_type_size(in.key_type) <= 4;
    const u32 S = g->S = agg_part_max_cells(ctx, agg_part_cell_bytes(a, in.key_type, n, &g->cnt32, word_pass ? agg_mask : ~0u));
    // partitions so that a partition's expected groups fill at most 70 % of the LDS table (fewer partitions = longer runs in
    // the scatter: an estimate of 1.25 M groups still gets 256 partitions)
    const u64 part_cap = (u64)S * 7 / 10;
    const u64 want_p = (in.size_hint + part_cap - 1) / part_cap;
    u32 P = 64;
    while (P < (u32)ctx->num_cus && P < GBP_MAX_P) // the aggregate pass runs one workgroup per partition: give every CU one
        P <<= 1;
    while (P < want_p && P < GBP_MAX_P)
        P <<= 1;
    // More groups than P_max partitions x half an LDS table: TWO LEVELS.  Level 1 cuts the rows into P1 big partitions with an
    // independent hash (long runs: close to a copy), then every big partition -- already in the 4/8-byte key + 8-byte word
    // layout -- goes through a level-2 call with its share of the promised groups.
    // (want_p already allows LDS tables 70 % full: up to ~5.9 M groups one level is the faster plan, 16 vs 24 ms at 5 M)
    if (want_p > GBP_MAX_P && level == 0 && !chgpu_opt(ctx, "tune_gb_no_two_level", 0))
    {
        const u64 sub_groups = (u64)(GBP_MAX_P / 2) * (S / 2); // leaves the second level at half its partition budget
        u32 P1 = 2;
        while ((u64)P1 * sub_groups < in.size_hint && P1 < 256)
            P1 <<= 1;
        if ((u64)P1 * sub_groups * 2 < in.size_hint || n / P1 < (1u << 20))
            return CHGPU_ERR_NOT_IMPLEMENTED; // beyond two levels, or partitions too small to be worth three passes each
        P = g->P1 = P1;
        g->mult = GBP_MULT1;
        level = 1;
    }
    else if (level == 0 && (u64)P * (S / 2) < in.size_hint / 4) // hopelessly more groups than P * S: partitioning would not localise them
        return CHGPU_ERR_NOT_IMPLEMENTED;
    g->level = level;
    g->P = P;
    // work units of the aggregate pass: half an average partition each, so a uniform input gives every workgroup two
    // units and a partition swollen by a hot key is spread over many workgroups; each unit flushes its LDS table once
    const u32 unit_div = (u32)chgpu_opt(ctx, "tune_gb_unitdiv", 2);
    g->chunk_rows = (n / ((u64)P * unit_div) + 63) / 64 * 64;
    if (g->chunk_rows < 65536)
        g->chunk_rows = 65536;
    g->max_units = n / g->chunk_rows + P;
    return CHGPU_OK;
}

// The table as the aggregate pass of `g` needs it: every unit's flush may claim up to S+1 cells without the max-fill check, so all of
// them must fit inside the slack.  size_hint: the promise of this call's rows (a table made here is sized from it).  Runs once the
// geometry is known and before the tile-sorted fit is tested, for a shape that is refused afterwards too: the capacity decides the
// row order of the results.
static int agg_partition_size_table(chgpu_agg * a, const GbPartPlan & g, u64 size_hint)
{
    if (g.level == 1) // a first partitioning level touches no table: its level-2 calls size it
        return CHGPU_OK;
    CHGPU_TRY(agg_ensure_table(a, size_hint, 2 * (g.max_units * (g.S + 1) + a->n_groups) + 2));
    for (int guard = 0; !a->t.find_only && guard < 16 && a->t.capacity / 2 < g.max_units * (g.S + 1) + a->n_groups; ++guard)
    {
        AggCtrl c0;
        CHGPU_TRY(agg_read_ctrl(a, &c0));
        CHGPU_TRY(agg_grow(a, c0.n_groups, c0.has_zero != 0));
    }
    return CHGPU_OK;
}

// The TILE-SORTED plan of a partitioned executeOnBlock (k_rp_tilesort + k_agg_tiles_lds): one level, one 8-byte argument column
// (or none besides counts), 4- or 8-byte keys, a compile-time state update.  Two passes over the rows instead of three (no histogram),
// and the partition pass writes whole lines in row order.
struct GbTilePlan
{
    size_t key_w = 0;
    u32 TILE = 0, n_tiles = 0;
    int arg_j = -1;      // the one argument column
    size_t arg_w = 0;    // as it is: 8-byte integers / Float64, or 4 bytes widened inside the partition pass
    int arg_ex = 0;      // that widening (EX of k_rp_tilesort): 3 = Int32, 4 = Float32, 0 = UInt32 or none
    u64 chunk_rows = 0;  // rows per work unit
    u32 max_units = 0;
    u32 cnt32 = 0;       // in the numbering of d
    u32 ops = 0;         // one of GbTileOps
    AggDesc d;           // localised to the pass's functions; argument pointers are set once the records are laid out
    u64 n_pad() const { return (u64)n_tiles * TILE; }
};

// NOT_IMPLEMENTED = the shape does not fit (the caller runs the scatter plan).
static int agg_tile_plan(const chgpu_agg * a, const AggInput & in, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 n,
                         const GbPartPlan & g, GbTilePlan * tp)
{
    const size_t key_w = tp->key_w = chgpu_type_size(in.key_type);
    if ((key_w != 4 && key_w != 8) || g.P > 512 || ((uintptr_t)key_col->data + row_begin * key_w) % 16 != 0)
        return CHGPU_ERR_NOT_IMPLEMENTED;
    const u32 TILE = tp->TILE = key_w == 4 ? 12288u : 8192u;
    if (n < (u64)TILE * a->ctx->num_cus || n + TILE >= (1ull << 32)) // (k_agg_tiles_lds indexes the sorted copy with 32 bits)
        return CHGPU_ERR_NOT_IMPLEMENTED;
    // the one argument column
    int arg_j = -1;
    for (u32 j = 0; j < a->n_aggs; ++j)
        if (a->kinds[j] != CHGPU_AGG_COUNT && ((g.agg_mask >> j) & 1))
        {
            if (arg_j >= 0 && arg_cols[j]->data != arg_cols[arg_j]->data)
                return CHGPU_ERR_NOT_IMPLEMENTED;
            if (arg_j < 0)
                arg_j = (int)j;
        }
    if (arg_j < 0)
        return CHGPU_ERR_NOT_IMPLEMENTED;
    const int arg_t = in.arg_types[arg_j];
    const size_t arg_w = tp->arg_w = chgpu_type_size(arg_t);
    tp->arg_j = arg_j;
    tp->arg_ex = arg_t == CHGPU_I32 ? 3 : arg_t == CHGPU_F32 ? 4 : 0;
    if ((arg_w != 8 && arg_w != 4) || ((uintptr_t)arg_cols[arg_j]->data + row_begin * arg_w) % (2 * arg_w) != 0)
        return CHGPU_ERR_NOT_IMPLEMENTED;
    tp->n_tiles = (u32)((n + TILE - 1) / TILE);
    // (6 % of slack on the unit size: the partitions of a uniform input all get the same number of units, so that units of equal rank
    //  cover equal stretches of tiles -- see k_tile_units)
    tp->chunk_rows = g.chunk_rows + g.chunk_rows / 16;
    tp->max_units = (u32)(n / tp->chunk_rows + g.P);
    // the aggregate pass reads the widened words of the sorted copy
    AggDesc & d = tp->d;
    agg_fill_desc(a, arg_cols, &d);
    for (u32 j = 0; j < a->n_aggs; ++j)
        if (a->kinds[j] != CHGPU_AGG_COUNT && ((g.agg_mask >> j) & 1))
        {
            d.a[j].arg_type = chgpu_type_is_float(in.arg_types[j]) ? CHGPU_F64 : CHGPU_U64;
            d.a[j].pre = 0;
        }
    tp->cnt32 = g.cnt32;
    if (g.agg_mask != ~0u)
    {
        agg_desc_keep(&d, g.agg_mask);
        agg_localise_words(&d, &tp->cnt32); // the pass's own state words 0 .. n-1 (a word pass sized S and P for exactly those)
    }
    tp->ops = agg_update_code(d, tp->cnt32);
    return GbTileOps::has(tp->ops) ? CHGPU_OK : CHGPU_ERR_NOT_IMPLEMENTED;
}

struct GbTileScratch
{
    unsigned long long * part_total; // [P] rows per partition
    u64 * unit_list;                 // [max_units + 1], then u32 unit_qstart[TILE_QUEUES + 1] and the queues' work counters u32 [TILE_QUEUES]
    u64 * pending;
    size_t zero_bytes;               // the three regions above: zeroed before the passes
    unsigned short * tidx;
    u32 * run_index;
    u64 * rec;                       // the sorted copy as {word, key} records (one piece per run and tile for the gather instead of two): the
                                     // key region and the word region of a structure-of-arrays copy taken together
    size_t bytes;
};

static GbTileScratch agg_tile_scratch(void * base, const GbTilePlan & tp, u32 P)
{
    ScratchCarver c{(uintptr_t)base};
    GbTileScratch s;
    s.part_total = c.take<unsigned long long>(P);
    s.unit_list = c.take<u64>((size_t)tp.max_units + 2 + 16);
    s.pending = c.take<u64>(tp.n_pad() / 64 + 1);
    s.zero_bytes = c.off;
    s.tidx = c.take<unsigned short>((size_t)tp.n_tiles * (P + 1) + 8);
    s.run_index = c.take<u32>((size_t)tp.n_tiles * P);
    s.rec = (u64 *)c.take<char>((size_t)tp.n_pad() * tp.key_w);
    (void)c.take<u64>(tp.n_pad());
    s.bytes = c.bytes();
    return s;
}

static int agg_tile_run(chgpu_agg * a, const AggInput & in, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 n,
                        const GbPartPlan & g, GbTilePlan & tp)
{
    static const char * const what = "tile-sorted aggregation";
    chgpu_ctx * ctx = a->ctx;
    const u32 P = g.P, S = g.S, n_tiles = tp.n_tiles;
    void * scratch = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, agg_tile_scratch(nullptr, tp, P).bytes, &scratch));
    const GbTileScratch s = agg_tile_scratch(scratch, tp, P);
    u32 * unit_qstart = (u32 *)(s.unit_list + tp.max_units + 1), * unit_ctr = unit_qstart + TILE_QUEUES + 1;
    AggDesc & d = tp.d;
    for (u32 m = 0; m < d.n_aggs; ++m)
        if (d.a[m].kind != CHGPU_AGG_COUNT)
            d.a[m].ptr = s.rec;
    const u32 G = (u32)ctx->num_cus;
    const u64 rows_per_wg = ((n + G - 1) / G + tp.TILE - 1) / tp.TILE * tp.TILE;
    if (chgpu_opt(ctx, "debug", 0))
        fprintf(stderr, "chgpu: tile-sorted GROUP BY n=%llu hint=%llu S=%u P=%u tile=%u ops=0x%x arg_w=%zu ex=%d\n", (unsigned long long)n, (unsigned long long)in.size_hint, S, P,
                tp.TILE, tp.ops, tp.arg_w, tp.arg_ex);
    CHGPU_HIP(hipMemsetAsync(scratch, 0, s.zero_bytes, ctx->stream));
    int rc = CHGPU_OK;
    dispatch_key(tp.key_w == 4, [&](auto kt) {
        using KT = decltype(kt);
        constexpr u32 TILE = sizeof(KT) == 4 ? 12288u : 8192u;
        auto sort = [&](auto at, auto ex) {
            using AT = decltype(at);
            rc = launch_lds(what, k_rp_tilesort<TILE, KT, GbpPartFn<KT>, RP_THREADS, AT, (int)decltype(ex)::value>, dim3(G), dim3(RP_THREADS),
                            rp_tilesort_lds_bytes(TILE, P, sizeof(KT)), ctx->stream, (const KT *)key_col->data + row_begin, (const AT *)arg_cols[tp.arg_j]->data + row_begin, n,
                            rows_per_wg, P, (KT *)s.rec, s.rec, s.tidx, s.part_total, GbpPartFn<KT>{P, GBP_MULT});
        };
        if (tp.arg_w == 8)
            sort(u64{}, std::integral_constant<u32, 0>{});
        else
            OneOf<0, 3, 4>::dispatch((u32)tp.arg_ex, [&](auto ex) { sort(u32{}, ex); });
        if (rc != CHGPU_OK)
            return;
        hipLaunchKernelGGL(k_tile_units, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned long long *)s.part_total, P, tp.chunk_rows, n_tiles, s.unit_list, tp.max_units, unit_qstart, unit_ctr);
        hipLaunchKernelGGL(k_tile_index_transpose, dim3((n_tiles + 63) / 64, (P + 63) / 64), dim3(256), 0, ctx->stream, (const unsigned short *)s.tidx, n_tiles, P, s.run_index);
        const size_t lds_ag = (size_t)PartLds(sizeof(KT), S, d.words.n_words, tp.cnt32).bytes() + 16;
        GbTileOps::dispatch(tp.ops, [&](auto ops) {
            rc = launch_lds(what, k_agg_tiles_lds<KT, decltype(ops)::value, TILE>, dim3(G), dim3(1024), lds_ag, ctx->stream, a->t, d, (const KT *)s.rec, (const u64 *)s.rec,
                            (const u32 *)s.run_index, n_tiles, P, s.pending, S, tp.cnt32, (const u64 *)s.unit_list, (const u32 *)unit_qstart, unit_ctr);
        });
    });
    ctx->counters[6] += 3;
    CHGPU_TRY(rc);
    return agg_finish_rounds_aos(a, d, (const u32 *)s.rec, tp.key_w == 4 ? 0 : 1, tp.n_pad(), s.pending);
}

// The scatter plan's launch shape for geometry `g`: tile and grid of the partition passes, whether the loads are wide, the descriptor
// of the aggregate pass over the partition buffers and its update code.
static void agg_scatter_plan(const chgpu_agg * a, const AggInput & in, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 n,
                             GbPartPlan * g)
{
    const chgpu_ctx * ctx = a->ctx;
    const u32 K = g->K, P = g->P;
    g->G = (u32)ctx->num_cus * GBP_WG_PER_CU;
    // the scatter's LDS image is tile*(8*K + key bytes) + 24*P bytes and must stay under ~159 KiB (160 KiB per workgroup, 64 B static)
    const size_t row_lds = 8 * K + (g->key32 ? 4 : 8);
    const u32 tile_cap = (u32)chgpu_opt(ctx, "tune_gb_tile", 12288);
    g->tile = 4096;
    for (u32 cand : {8192u, 12288u})
        if (cand <= tile_cap && cand * row_lds + (size_t)P * 24 + 64 <= 159 * 1024)
            g->tile = cand;
    g->rows_per_wg = ((n + g->G - 1) / g->G + g->tile - 1) / g->tile * g->tile;
    // the argument columns of this call's functions in the order of their words in the partition buffers; the aggregate pass reads the
    // widened 8-byte words: integers were sign/zero-extended, Float64 kept its bits
    g->gc.k = K;
    agg_fill_desc(a, arg_cols, &g->d);
    u32 kk = 0;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        if (a->kinds[j] == CHGPU_AGG_COUNT || !((g->agg_mask >> j) & 1))
            continue;
        g->gc.src[kk] = arg_cols[j]->data;
        g->gc.type[kk] = in.arg_types[j];
        g->d.a[j].arg_type = chgpu_type_is_float(in.arg_types[j]) ? CHGPU_F64 : CHGPU_U64;
        g->d.a[j].pre = kk++;
    }
    if (g->agg_mask != ~0u)
        agg_desc_keep(&g->d, g->agg_mask);
    // wide loads need key/argument columns whose element width is the buffer width and a 16-byte aligned first row
    const size_t key_w = chgpu_type_size(in.key_type);
    bool wide = (key_w == 4 || key_w == 8) && ((uintptr_t)key_col->data + row_begin * key_w) % 16 == 0;
    for (u32 c = 0; c < K; ++c)
        wide = wide && chgpu_type_size(g->gc.type[c]) == 8 && ((uintptr_t)g->gc.src[c] + row_begin * 8) % 16 == 0;
    g->wide = wide && !chgpu_opt(ctx, "tune_gb_nowide", 0);
    // the branch-free scatter (radix_partition.h): one 8-byte word, wide loads
    g->rp_tile = 0;
    if (g->wide && K == 1 && n + RP_SCATTER_SLACK < (1ull << 32) && P + 1 <= 2 * RP_THREADS)
        g->rp_tile = g->key32 && rp_scatter_lds_bytes(12288, P, 4, true) <= 159 * 1024 ? 12288 : 8192;
    // the update of the state words as a compile-time code where the common shapes allow it
    g->ops = chgpu_opt(ctx, "tune_gb_noops", 0) ? 0 : agg_update_code(g->d, g->cnt32);
    if (!GbPartOps::has(g->ops))
        g->ops = 0;
}

struct GbScatterScratch
{
    u32 * counts;     // [P * G] rows per partition and workgroup
    u64 * offsets;    // [P * G + 1] their exclusive scan
    u64 * total_dev;
    void * tmp;       // the scan's
    size_t tmp_b;
    u64 * pending;    // one bit per row, then u32 unit_start[GBP_MAX_P + 1] and the work counter
    u32 * unit_start;
    size_t pend_b;    // pending and unit_start together: zeroed before the aggregate pass
    void * pkeys;     // the partition buffers: keys (4 or 8 B) | word0 | word1, each of `wstride` rows
    u64 * pwords;
    u64 wstride;
    size_t bytes;
};

// m = P * G counters; n rows of K argument words
static GbScatterScratch agg_scatter_scratch(void * base, u64 m, u64 n, u32 K, bool key32)
{
    ScratchCarver c{(uintptr_t)base};
    GbScatterScratch s;
    s.counts = c.take<u32>(m);
    s.offsets = c.take<u64>(m + 1);
    s.total_dev = c.take<u64>(1);
    s.tmp_b = chgpu_scan_tmp_bytes(m);
    s.tmp = c.take_packed<char>(s.tmp_b);
    const size_t pend_off = c.off;
    s.pending = c.take<u64>((n + 63) / 64 + 1);
    s.unit_start = c.take<u32>(GBP_MAX_P + 2);
    s.pend_b = c.off - pend_off;
    // The partition buffers live in the context's scratch arena, which is kept between calls: a fresh hipMalloc of
    // 16 GB costs ~0.4 s, fifteen times the kernels it would serve.
    s.wstride = n + RP_SCATTER_SLACK; // rows per array (k_rp_scatter parks out-of-range rows in the slack)
    s.pkeys = c.take<char>((size_t)s.wstride * (key32 ? 4 : 8));
    s.pwords = c.take<u64>((size_t)s.wstride * K);
    s.bytes = c.bytes();
    return s;
}

static int agg_add_block_partitioned(chgpu_agg * a, const AggInput & in, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 n, u32 K,
                                     int level = 0, size_t scratch_off = 0, u32 agg_mask = ~0u);

// Level 1 of the two-level plan, after its scatter: every big partition -- a slice of the partition buffers `s` -- goes through a
// level-2 call with its share of the promised groups; their scratch starts at sub_off, behind this level's own.
static int agg_partitioned_level2(chgpu_agg * a, const AggInput & in, const GbPartPlan & g, const GbScatterScratch & s, u64 n, size_t sub_off)
{
    chgpu_ctx * ctx = a->ctx;
    const u32 P1 = g.P1;
    // partition boundaries: offsets[p * G] for p = 0..P1-1 (the read-back also orders the host behind the scatter)
    std::vector<u64> starts(P1 + 1);
    void * stage = nullptr;
    CHGPU_TRY(chgpu_pinned(ctx, (size_t)P1 * 8, &stage));
    CHGPU_HIP(hipMemcpy2DAsync(stage, 8, s.offsets, (size_t)g.G * 8, 8, P1, hipMemcpyDeviceToHost, ctx->stream));
    CHGPU_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(starts.data(), stage, (size_t)P1 * 8);
    starts[P1] = n;
    // the partition buffers as columns: keys of the buffer width, arguments widened to 8 bytes (Float64 kept its bits)
    chgpu_col kc{};
    kc.ctx = ctx;
    kc.type = g.key32 ? CHGPU_U32 : CHGPU_U64;
    kc.rows = n;
    kc.data = s.pkeys;
    chgpu_col ac[GBP_MAX_K]{};
    const chgpu_col * sub_args[AGG_MAX_AGGS] = {};
    AggInput sub = in;
    sub.key_type = kc.type;
    sub.size_hint = in.size_hint / P1 + in.size_hint / P1 / 4 + 1024;
    u32 c = 0;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        if (a->kinds[j] == CHGPU_AGG_COUNT || !((g.agg_mask >> j) & 1))
            continue;
        ac[c].ctx = ctx;
        ac[c].type = sub.arg_types[j] = chgpu_type_is_float(in.arg_types[j]) ? CHGPU_F64 : CHGPU_U64; // two's complement sums: width is what matters
        ac[c].rows = n;
        ac[c].data = s.pwords + (u64)c * s.wstride;
        sub_args[j] = &ac[c];
        ++c;
    }
    for (u32 q = 0; q < P1; ++q)
        if (starts[q + 1] > starts[q])
            CHGPU_TRY(agg_add_block_partitioned(a, sub, &kc, sub_args, starts[q], starts[q + 1] - starts[q], g.K, 2, sub_off, g.agg_mask));
    return CHGPU_OK;
}

// The scatter plan: histogram, scan, scatter into the partition buffers, then the LDS aggregate pass over them (or, at level 1, a
// level-2 call per big partition).
static int agg_scatter_run(chgpu_agg * a, const AggInput & in, const chgpu_col * key_col, u64 row_begin, u64 n, GbPartPlan & g, size_t scratch_off)
{
    static const char * const what = "partitioned aggregation";
    chgpu_ctx * ctx = a->ctx;
    const u32 K = g.K, P = g.P, G = g.G, S = g.S;
    const u64 mult = g.mult, rows_per_wg = g.rows_per_wg;
    if (chgpu_opt(ctx, "debug", 0))
        fprintf(stderr, "chgpu: partitioned GROUP BY level=%d n=%llu hint=%llu S=%u P=%u G=%u tile=%u ops=0x%x wide=%d rp_tile=%u\n", g.level, (unsigned long long)n,
                (unsigned long long)in.size_hint, S, P, G, g.tile, g.ops, g.wide ? 1 : 0, g.rp_tile);
    const u64 m = (u64)P * G;
    const size_t own_b = agg_scatter_scratch(nullptr, m, n, K, g.key32).bytes;
    // a level-1 call reserves the region of its level-2 calls up front (growing the arena later would move it): the same
    // row count at most, bookkeeping for the largest partition count
    const size_t sub_b = g.level == 1 ? agg_scatter_scratch(nullptr, (u64)GBP_MAX_P * G, n, K, g.key32).bytes + 4096 : 0;
    void * scratch_base = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, scratch_off + own_b + sub_b, &scratch_base));
    const GbScatterScratch s = agg_scatter_scratch((char *)scratch_base + scratch_off, m, n, K, g.key32);
    for (u32 c = 0; c < K; ++c)
        g.gc.dst[c] = s.pwords + (u64)c * s.wstride;
    AggDesc & d = g.d;
    for (u32 j = 0; j < d.n_aggs; ++j)
        if (d.a[j].kind != CHGPU_AGG_COUNT)
            d.a[j].ptr = g.gc.dst[d.a[j].pre];

    if (g.wide)
        dispatch_key(g.key32, [&](auto kt) {
            using KT = decltype(kt);
            hipLaunchKernelGGL((k_rp_hist_wide<KT, GbpPartFn<KT>>), dim3(G), dim3(RP_THREADS), 0, ctx->stream, (const KT *)key_col->data + row_begin, n, rows_per_wg, P, s.counts,
                               GbpPartFn<KT>{P, mult});
        });
    else
        hipLaunchKernelGGL(k_gb_hist, dim3(G), dim3(GBP_THREADS), 0, ctx->stream, (const void *)key_col->data, in.key_type, row_begin, n, rows_per_wg, P, s.counts, mult, g.key32 ? 1 : 0);
    int rc = chgpu_scan_exclusive_u32_u64(ctx, s.counts, s.offsets, m, s.total_dev, s.tmp, s.tmp_b);
    if (rc == CHGPU_OK)
        dispatch_key(g.key32, [&](auto kt) {
            using KT = decltype(kt);
            if (g.rp_tile)
            {
                using Tiles = std::conditional_t<sizeof(KT) == 4, OneOf<12288, 8192>, OneOf<8192>>;
                Tiles::dispatch(g.rp_tile, [&](auto t) {
                    constexpr u32 TILE = decltype(t)::value;
                    rc = launch_lds(what, k_rp_scatter<TILE, KT, true, GbpPartFn<KT>>, dim3(G), dim3(RP_THREADS), rp_scatter_lds_bytes(TILE, P, sizeof(KT), true), ctx->stream,
                                    (const KT *)key_col->data + row_begin, (const u64 *)g.gc.src[0] + row_begin, n, rows_per_wg, P, (const u64 *)s.offsets, (KT *)s.pkeys,
                                    g.gc.dst[0], GbpPartFn<KT>{P, mult});
                });
                return;
            }
            const size_t lds_sc = (size_t)g.tile * (8 * K + sizeof(KT)) + (size_t)P * 24 + 64;
            OneOf<4096, 8192, 12288>::dispatch(g.tile, [&](auto t) {
                dispatch_const<0, 1>(g.wide ? 1 : 0, [&](auto w) {
                    rc = launch_lds(what, k_gb_scatter<decltype(t)::value, KT, decltype(w)::value != 0>, dim3(G), dim3(GBP_THREADS), lds_sc, ctx->stream,
                                    (const void *)key_col->data, in.key_type, row_begin, n, rows_per_wg, P, (const u64 *)s.offsets, g.gc, (KT *)s.pkeys, mult);
                });
            });
        });
    if (g.level == 1)
    {
        ctx->counters[6] += 2;
        CHGPU_TRY(rc);
        return agg_partitioned_level2(a, in, g, s, n, scratch_off + own_b);
    }
    if (rc == CHGPU_OK && hipMemsetAsync(s.pending, 0, s.pend_b, ctx->stream) != hipSuccess)
        rc = chgpu_set_error(CHGPU_ERR_DEVICE, "%s: clearing the pending rows failed", what);
    if (rc == CHGPU_OK)
    {
        u32 * unit_ctr = s.unit_start + GBP_MAX_P + 1;
        hipLaunchKernelGGL(k_gb_units, dim3(1), dim3(1024), 0, ctx->stream, (const u64 *)s.offsets, G, P, n, g.chunk_rows, s.unit_start, unit_ctr);
        dispatch_key(g.key32, [&](auto kt) {
            using KT = decltype(kt);
            const size_t lds_ag = (size_t)PartLds(sizeof(KT), S, a->words.n_words, g.cnt32).bytes() + 16; // the kernel zeroes whole 8-byte words
            auto launch = [&](auto ops) {
                rc = launch_lds(what, k_agg_part_lds<KT, 8, KT, false, decltype(ops)::value>, dim3((u32)ctx->num_cus), dim3(1024), lds_ag, ctx->stream, a->t, d, (const KT *)s.pkeys,
                                (const void *)s.pwords, (const void *)(s.pwords + s.wstride), (const u64 *)s.offsets, G, P, n, s.pending, S, K, g.cnt32, g.chunk_rows,
                                (const u32 *)s.unit_start, unit_ctr, (const u8 *)nullptr, (const u8 *)nullptr, 0u);
            };
            if (!GbPartOps::dispatch(g.ops, launch))
                launch(std::integral_constant<u32, 0>{}); // the update read from the descriptor
        });
    }
    ctx->counters[6] += 3;
    CHGPU_TRY(rc);
    return agg_finish_rounds(a, d, s.pkeys, g.key32 ? CHGPU_U32 : CHGPU_U64, 0, n, s.pending);
}

// PARTITIONED executeOnBlock (see the kernel block comment).  Returns NOT_IMPLEMENTED when the shape does not fit
// (the caller then uses the DIRECT kernel).
// level 0: called by add_block; may turn itself into level 1 (the first of two partitioning levels: partitions the rows
// into P1 big partitions and runs a level-2 call over each partition buffer slice); level 2 never recurses.
// agg_mask: the aggregate functions this call applies (bit j = function j); the caller splits more than GBP_MAX_K argument
// columns into several calls over the same rows, each partitioning the key column with its own two argument columns.
static int agg_add_block_partitioned(chgpu_agg * a, const AggInput & in, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 n, u32 K,
                                     int level, size_t scratch_off, u32 agg_mask)
{
    GbPartPlan g;
    CHGPU_TRY(agg_partition_geometry(a, in, n, K, level, agg_mask, false, &g));
    CHGPU_TRY(agg_partition_size_table(a, g, in.size_hint));
    // one level, one argument word: the tile-sorted plan (two passes, streaming writes) where its shape fits
    if (g.level == 0 && K == 1 && !chgpu_opt(a->ctx, "tune_gb_no_tiled", 0))
    {
        GbTilePlan tp;
        if (agg_tile_plan(a, in, key_col, arg_cols, row_begin, n, g, &tp) == CHGPU_OK)
            return agg_tile_run(a, in, key_col, arg_cols, row_begin, n, g, tp);
    }
    agg_scatter_plan(a, in, key_col, arg_cols, row_begin, n, &g);
    return agg_scatter_run(a, in, key_col, row_begin, n, g, scratch_off);
}

// One pass of a per-word GROUP BY: the functions of `agg_mask` (one argument word, perhaps the counts) through the tile-sorted plan,
// with partitions and LDS cells sized for their state words alone.  launch = false only asks whether the plan takes the pass; the
// table is sized either way (see agg_partition_size_table).  NOT_IMPLEMENTED = it does not (a pass sized for this plan has no other).
static int agg_word_pass(chgpu_agg * a, const AggInput & in, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 n, u32 agg_mask,
                         bool launch)
{
    GbPartPlan g;
    CHGPU_TRY(agg_partition_geometry(a, in, n, 1, 0, agg_mask, true, &g));
    CHGPU_TRY(agg_partition_size_table(a, g, in.size_hint));
    if (g.level != 0)
        return CHGPU_ERR_NOT_IMPLEMENTED;
    GbTilePlan tp;
    CHGPU_TRY(agg_tile_plan(a, in, key_col, arg_cols, row_begin, n, g, &tp));
    return launch ? agg_tile_run(a, in, key_col, arg_cols, row_begin, n, g, tp) : CHGPU_OK;
}

// The functions that take an argument, `per_call` at a time in their order, as one mask per call (ks[c]: how many the call carries);
// every count() rides in the first.  Returns the number of calls.
static u32 agg_split_calls(const chgpu_agg * a, u32 per_call, u32 * masks, u32 * ks)
{
    u32 n_calls = 0;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        if (a->kinds[j] == CHGPU_AGG_COUNT)
            continue;
        if (n_calls == 0 || ks[n_calls - 1] == per_call)
            masks[n_calls] = 0, ks[n_calls] = 0, ++n_calls;
        masks[n_calls - 1] |= 1u << j;
        ++ks[n_calls - 1];
    }
    if (n_calls)
        masks[0] |= agg_count_mask(a);
    return n_calls;
}

// PARTITIONED strategy: large promised cardinality and enough rows to amortise two extra passes
static bool agg_partition_gate(const chgpu_agg * a, u64 lds_groups, u64 n)
{
    return a->size_hint > lds_groups && n >= (4u << 20) && !chgpu_opt(a->ctx, "agg_no_partition", 0);
}

// The partitioned plans come first for such a block, unless its states are not additive (min / max / any: the LDS-staged and partitioned
// plans carry additive words only) or carry a per-function mask (the partition buffers have none)
static bool agg_tries_partitions(const chgpu_agg * a, u64 lds_groups, u64 n)
{
    return !a->has_extremum && !a->conditioned && agg_partition_gate(a, lds_groups, n);
}
// Does the block take the RANGE-mode kernel (agg_add_block_ranged) -- the only plan a WHERE mask is fused into?  It does when the
// partitioned plans are not tried, or were and refused the shape (partitions_refused: known only once they were asked), and the states
// are additive with few enough promised groups for a workgroup's LDS table.  Keys of 1, 2, 4 or 8 bytes: every key type.
static bool agg_takes_ranged(const chgpu_agg * a, u64 lds_groups, u64 n, bool partitions_refused = false)
{
    return (partitions_refused || !agg_tries_partitions(a, lds_groups, n)) && !a->has_extremum &&
           a->size_hint <= 65536 /* beyond that nearly every key misses a workgroup's LDS table */ && n < (1ull << 32) &&
           !chgpu_opt(a->ctx, "tune_agg_no_ranged", 0);
}

// The partitioned plans for a block that passed agg_partition_gate.  NOT_IMPLEMENTED: no plan takes the shape and nothing was added.
static int agg_add_block_by_partitions(chgpu_agg * a, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 n)
{
    chgpu_ctx * ctx = a->ctx;
    const AggInput in = agg_input_of(a);
    u32 masks[AGG_MAX_AGGS], ks[AGG_MAX_AGGS];
    const u32 n_argwords = agg_split_calls(a, 1, masks, ks);
    // Two or more argument words: ONE PASS PER WORD through the tile-sorted plan (each pass sorts {key, its word} and aggregates into
    // cells that hold only its own state words; every count() rides in the first) -- 7 ms per word and 1e9 rows, against 22 ms for
    // the two-word scatter plan, whose 4096-row tiles leave 8-row runs (tools/bench_two_words.py).  A shape the plan does not take
    // answers NOT_IMPLEMENTED when asked, before anything was added: the older routes below take over.
    if (n_argwords >= 2 && !chgpu_opt(ctx, "tune_gb_no_tiled", 0) && !chgpu_opt(ctx, "tune_gb_no_word_passes", 0))
    {
        // every pass is asked first whether the plan takes it (nothing may be added before all of them are known to run)
        int rc = CHGPU_OK;
        for (u32 c = 0; c < n_argwords && rc == CHGPU_OK; ++c)
            rc = agg_word_pass(a, in, key_col, arg_cols, row_begin, n, masks[c], false);
        for (u32 c = 0; c < n_argwords && rc == CHGPU_OK; ++c)
        {
            rc = agg_word_pass(a, in, key_col, arg_cols, row_begin, n, masks[c], true);
            if (rc == CHGPU_ERR_NOT_IMPLEMENTED) // (the plan said yes when asked: not reached)
                return chgpu_set_error(CHGPU_ERR_LOGICAL, "a pass of a per-word GROUP BY was refused after its probe");
        }
        if (rc != CHGPU_ERR_NOT_IMPLEMENTED)
            return rc;
    }
    if (n_argwords <= GBP_MAX_K)
        return agg_add_block_partitioned(a, in, key_col, arg_cols, row_begin, n, n_argwords);
    // more argument columns than a partition buffer row carries: several partitioned calls over the same rows, each with
    // two of them (plus every count() in the first) -- ~12 ms per 1e9 rows and call, against one HBM atomic per row
    // and state word on the DIRECT path
    const u32 n_calls = agg_split_calls(a, GBP_MAX_K, masks, ks);
    int rc = CHGPU_OK;
    for (u32 c = 0; c < n_calls && rc == CHGPU_OK; ++c)
        rc = agg_add_block_partitioned(a, in, key_col, arg_cols, row_begin, n, ks[c], 0, 0, masks[c]);
    return rc; // (NOT_IMPLEMENTED comes from the first call, before anything was applied: the caller takes the other strategies)
}

static int agg_add_block_impl(chgpu_agg * a, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 row_end,
                              const chgpu_col * filter);

// the calls that carry no condition columns, on an aggregator whose functions need them
#define AGG_REQUIRE_UNCONDITIONED(a)                                                                                   \
    CHGPU_REQUIRE(!(a) || !(a)->conditioned, CHGPU_ERR_BAD_ARGUMENTS, "the aggregator has conditioned functions: use chgpu_agg_execute_on_block_conditional")

extern "C" int chgpu_agg_add_block(chgpu_agg * a, const chgpu_col * key_col, const chgpu_col * const * arg_cols,
                                   uint64_t row_begin, uint64_t row_end)
{
    ChgpuDeviceGuard _dev_guard(a ? a->ctx : nullptr);
    AGG_REQUIRE_UNCONDITIONED(a);
    return agg_add_block_impl(a, key_col, arg_cols, row_begin, row_end, nullptr);
}

extern "C" int chgpu_agg_add_block_filtered(chgpu_agg * a, const chgpu_col * key_col, const chgpu_col * const * arg_cols,
                                            uint64_t row_begin, uint64_t row_end, const chgpu_col * filter_u8)
{
    ChgpuDeviceGuard _dev_guard(a ? a->ctx : nullptr);
    AGG_REQUIRE_UNCONDITIONED(a);
    return agg_add_block_impl(a, key_col, arg_cols, row_begin, row_end, filter_u8);
}

// The strategies that have no fused form: FilterTransform's work is done first (every column of the block filtered by the
// mask, chgpu_filter_columns) and the filtered block aggregated.
static int agg_add_block_materialised(chgpu_agg * a, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 row_end,
                                      const chgpu_col * filter)
{
    chgpu_ctx * ctx = a->ctx;
    const u64 n = row_end - row_begin;
    const chgpu_col * src[1 + 3 * AGG_MAX_AGGS];
    chgpu_col * views[2 + 3 * AGG_MAX_AGGS] = {};
    u32 m = 0;
    int rc = CHGPU_OK;
    auto view = [&](const chgpu_col * c) {
        if (rc == CHGPU_OK)
            rc = chgpu_col_slice(ctx, c, row_begin, n, &views[m]);
        if (rc == CHGPU_OK)
            ++m;
    };
    view(filter);
    view(key_col);
    u32 data_of[2 * AGG_MAX_AGGS]; // by argument slot (an argMin / argMax carries both its columns)
    for (u32 j = 0; j < a->n_aggs; ++j)
        for (u32 sl = a->slot[j]; sl < agg_slot_end(a, j); ++sl)
        {
            data_of[sl] = m - 1; // index among the data columns (key = 0)
            view(arg_cols[sl]);
        }
    // the condition columns travel with the keys and arguments (each distinct column once)
    u32 cond_of[AGG_MAX_AGGS], cond_first[AGG_MAX_AGGS];
    const chgpu_col * const * conds = a->conditioned ? a->block_conds : nullptr;
    const u32 n_conds = conds ? agg_number_conds(a, false, cond_of, cond_first) : 0;
    const u32 cond0 = m - 1; // condition column c is data column cond0 + c
    for (u32 c = 0; c < n_conds; ++c)
        view(conds[cond_first[c]]);
    chgpu_col * outs[1 + 3 * AGG_MAX_AGGS] = {};
    u64 kept = 0;
    const u32 n_data = m ? m - 1 : 0;
    if (rc == CHGPU_OK)
    {
        for (u32 k = 0; k < n_data; ++k)
            src[k] = views[1 + k];
        rc = chgpu_filter_columns(ctx, n_data, src, views[0], -1, outs, &kept);
    }
    if (rc == CHGPU_OK && kept)
    {
        const chgpu_col * fargs[2 * AGG_MAX_AGGS] = {};
        for (u32 j = 0; j < a->n_aggs; ++j)
            for (u32 sl = a->slot[j]; sl < agg_slot_end(a, j); ++sl)
                fargs[sl] = outs[data_of[sl]];
        const chgpu_col * fconds[AGG_MAX_AGGS] = {};
        for (u32 j = 0; conds && j < a->n_aggs; ++j)
            if (a->cond_modes[j] != CHGPU_AGG_COND_NONE)
                fconds[j] = outs[cond0 + cond_of[j]];
        if (conds)
            a->block_conds = fconds;
        rc = agg_add_block_impl(a, outs[0], fargs, 0, kept, nullptr);
        if (conds)
            a->block_conds = conds;
    }
    for (u32 k = 0; k < n_data; ++k)
        chgpu_col_free(outs[k]);
    for (u32 k = 0; k < m; ++k)
        chgpu_col_free(views[k]);
    return rc;
}

// without key: out[i] = filter[i] (NULL: 1) AND ((cond[i] != 0) == want) over rows [row_begin, row_begin + n), indexed like the columns
__global__ __launch_bounds__(256) void k_nokey_cond_mask(const u8 * __restrict__ filter, const u8 * __restrict__ cond, int want, u64 row_begin, u64 n,
                                                         u8 * __restrict__ out)
{
    for (u64 r = (u64)blockIdx.x * 256 + threadIdx.x; r < n; r += (u64)gridDim.x * 256)
    {
        const u64 i = row_begin + r;
        out[i] = (u8)((!filter || filter[i]) && (int)(cond[i] != 0) == want);
    }
}

// executeWithoutKeyImpl (Aggregator.cpp:1276-1321): addBatchSinglePlace per function
static int agg_add_nokey(chgpu_agg * a, const chgpu_col * const * arg_cols, u64 row_begin, u64 row_end, const chgpu_col * filter)
{
    chgpu_ctx * ctx = a->ctx;
    const u64 n = row_end - row_begin;
    u64 kept = n;
    if (filter)
    {
        // addBatchSinglePlace under a condition (addManyConditional, AggregateFunctionSum.h:138-236); count = countBytesInFilter
        chgpu_col * fv = nullptr;
        CHGPU_TRY(chgpu_col_slice(ctx, filter, row_begin, n, &fv));
        const int rc = chgpu_count_bytes_in_filter(ctx, fv, &kept);
        chgpu_col_free(fv);
        CHGPU_TRY(rc);
    }
    // A one-word reduction: the word is filled with the byte `fill` (< 0: left as it is), `launch(word)` starts the kernel, *out = the word
    auto reduce_word = [&](int fill, auto launch, u64 * out) -> int {
        void * scratch = nullptr;
        CHGPU_TRY(chgpu_scratch(ctx, 256, &scratch));
        if (fill >= 0)
            CHGPU_HIP(hipMemsetAsync(scratch, fill, 8, ctx->stream));
        launch((unsigned long long *)scratch);
        ctx->counters[6] += 1;
        CHGPU_HIP(hipGetLastError());
        return chgpu_read_back(ctx, scratch, out, 8);
    };
    const u32 grid = chgpu_grid_for(ctx, n, 256, 8);
    // one function under one mask (`filter`, which lets `kept` rows through)
    auto add_function = [&](u32 j, const chgpu_col * filter, u64 kept) -> int {
        const int kind = a->kinds[j];
        const AggKind & k = agg_kind(kind);
        u64 * st = &a->host_words[a->word_off[j]];
        const chgpu_col * col = k.slots ? arg_cols[a->slot[j]] : nullptr;
        const u8 * cond = filter ? (const u8 *)filter->data : nullptr;
        // the value of row `row` of the block, as the function's argument column holds it
        auto load_arg = [&](u64 row, u64 * bits) {
            return reduce_word(-1, [&](unsigned long long * dev) {
                hipLaunchKernelGGL(k_nokey_load, dim3(1), dim3(64), 0, ctx->stream, (const void *)col->data, a->arg_types[j], row_begin + row, (u64 *)dev);
            }, bits);
        };
        if (kind == CHGPU_AGG_COUNT)
            st[0] += kept;
        else if (k.extremum && (kept == 0 || n == 0))
            return CHGPU_OK;
        else if (k.slots == 2)
        {
            // the block's lexicographic extremum of (val key, ~ordinal): the largest val key, its first holder, that row's arg
            const chgpu_col * val = arg_cols[a->slot[j] + 1];
            const int is_min = kind == CHGPU_AGG_ARG_MIN ? 1 : 0;
            u64 best = 0, first = ~0ull, bits = 0;
            CHGPU_TRY(reduce_word(0, [&](unsigned long long * dev) {
                hipLaunchKernelGGL(k_nokey_extremum, dim3(grid), dim3(256), 0, ctx->stream, (const void *)val->data, a->val_types[j], row_begin, n, cond, is_min, 1, dev);
            }, &best));
            if (st[1] != 0 && best <= st[0])
                return CHGPU_OK; // setIfGreater / setIfSmaller: only a strictly better val replaces a state that has a value
            CHGPU_TRY(reduce_word(0xFF, [&](unsigned long long * dev) {
                hipLaunchKernelGGL(k_nokey_first_holder, dim3(grid), dim3(256), 0, ctx->stream, (const void *)val->data, a->val_types[j], row_begin, n, cond, is_min, best, dev);
            }, &first));
            CHGPU_REQUIRE(first != ~0ull, CHGPU_ERR_LOGICAL, "argMin / argMax: no row holds the block's extremum");
            CHGPU_TRY(load_arg(first, &bits));
            st[0] = best;
            st[1] = agg_arg_row_claim(a->any_seq + first);
            st[2] = bits;
        }
        else if (kind == CHGPU_AGG_ANY)
        {
            if (st[0] != 0) // setIfFirst: only a state without a value takes one
                return CHGPU_OK;
            u64 v = 0, bits = 0;
            CHGPU_TRY(reduce_word(0xFF, [&](unsigned long long * dev) {
                hipLaunchKernelGGL(k_nokey_first_row, dim3(grid), dim3(256), 0, ctx->stream, row_begin, n, cond, dev);
            }, &v));
            CHGPU_REQUIRE(v != ~0ull, CHGPU_ERR_LOGICAL, "any: none of the %llu rows the mask keeps was found", (unsigned long long)kept);
            CHGPU_TRY(load_arg(v, &bits));
            st[0] = ~(a->any_seq + v);
            st[1] = bits;
        }
        else if (k.extremum)
        {
            u64 v = 0;
            CHGPU_TRY(reduce_word(0, [&](unsigned long long * dev) {
                hipLaunchKernelGGL(k_nokey_extremum, dim3(grid), dim3(256), 0, ctx->stream, (const void *)col->data, a->arg_types[j], row_begin, n, cond,
                                   kind == CHGPU_AGG_MIN ? 1 : 0, 0, dev);
            }, &v));
            st[0] = v > st[0] ? v : st[0]; // order keys under an unsigned max (see agg_order_key); zero = no value yet
        }
        else
        {
            if (filter)
                CHGPU_TRY(chgpu_sum_add_many_conditional(ctx, col, filter, row_begin, row_end, st));
            else
                CHGPU_TRY(chgpu_sum_add_many(ctx, col, row_begin, row_end, st));
            if (kind == CHGPU_AGG_AVG)
                st[1] += kept;
        }
        return CHGPU_OK;
    };
    // every function aggregates under `filter AND its own condition` (-If: the byte is non-zero, Nullable: the null-map byte is zero)
    const chgpu_col * const * conds = a->conditioned ? a->block_conds : nullptr;
    chgpu_col * masks[AGG_MAX_AGGS] = {};
    u64 mask_kept[AGG_MAX_AGGS] = {};
    u32 mask_of[AGG_MAX_AGGS], mask_first[AGG_MAX_AGGS]; // functions with the same column and mode share the mask of the first of them
    if (conds)
        (void)agg_number_conds(a, true, mask_of, mask_first);
    int rc = CHGPU_OK;
    for (u32 j = 0; j < a->n_aggs && rc == CHGPU_OK; ++j)
    {
        if (!conds || a->cond_modes[j] == CHGPU_AGG_COND_NONE)
        {
            rc = add_function(j, filter, kept);
            continue;
        }
        const u32 src = mask_first[mask_of[j]];
        if (src == j && n)
        {
            rc = chgpu_col_new(ctx, CHGPU_U8, row_end, &masks[j]);
            if (rc != CHGPU_OK)
                break;
            hipLaunchKernelGGL(k_nokey_cond_mask, dim3(grid), dim3(256), 0, ctx->stream, filter ? (const u8 *)filter->data : nullptr,
                               (const u8 *)conds[j]->data, a->cond_modes[j] == CHGPU_AGG_COND_IF ? 1 : 0, row_begin, n, (u8 *)masks[j]->data);
            ctx->counters[6] += 1;
            chgpu_col * mv = nullptr;
            rc = chgpu_col_slice(ctx, masks[j], row_begin, n, &mv);
            if (rc == CHGPU_OK)
            {
                rc = chgpu_count_bytes_in_filter(ctx, mv, &mask_kept[j]);
                chgpu_col_free(mv);
            }
            if (rc != CHGPU_OK)
                break;
        }
        if (n)
            rc = add_function(j, masks[src], mask_kept[src]);
        const u32 seen_w = a->word_off[j] + agg_kind(a->kinds[j]).words;
        if (rc == CHGPU_OK && ((a->words.seen >> seen_w) & 1))
            a->host_words[seen_w] += mask_kept[src];
    }
    for (u32 j = 0; j < a->n_aggs; ++j)
        if (masks[j])
            chgpu_col_free(masks[j]);
    CHGPU_TRY(rc);
    a->any_seq += n;
    a->nokey_kept += kept;
    return CHGPU_OK;
}

// RANGE mode of the partition-aggregate kernel: 4/8-byte keys; a launch takes at most GBP_MAX_K argument columns of one
// width (8, 4 or 1 B), so the aggregate functions are split into PASSES over the same rows -- each pass re-reads the key
// column and updates its own state words of the same groups (TPC-H Q1's seven sums and averages: 4 passes x ~20 B/row
// instead of one trip through the generic kernel, which is 6x slower per row).
static int agg_add_block_ranged(chgpu_agg * a, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 n, const chgpu_col * filter,
                                const AggDesc & d, u64 * pending, u64 n_words64, u32 lds_cells)
{
    chgpu_ctx * ctx = a->ctx;
    struct Pass
    {
        u32 n = 0;           // argument columns in this pass
        u32 agg[GBP_MAX_K];  // their aggregate indices
        size_t aw = 8;       // their width
        bool ext = false;    // one of them is a signed narrow integer or Float32
        int cond = -1;       // the condition column its functions share (index into d.cond; -1: unconditioned) ...
        u32 want = 0;        // ... and what its non-zero test must give
        u32 counts = 0;      // the count() functions that ride in it (bit j)
    };
    // Functions are grouped by argument width AND condition: a pass carries at most one per-function mask.  count() needs no argument:
    // it rides in the first pass under its own condition (countIf(c) with a sumIf(x, c)), or gets an argument-less pass.
    Pass passes[AGG_MAX_AGGS];
    u32 n_passes = 0;
    for (int counts = 0; counts < 2; ++counts)
        for (u32 j = 0; j < a->n_aggs; ++j)
        {
            if ((a->kinds[j] == CHGPU_AGG_COUNT) != (counts != 0))
                continue;
            const size_t w = chgpu_type_size(a->arg_types[j]);
            u32 p = 0;
            for (; p < n_passes; ++p) // first pass of this condition (and, for an argument, of its width with a free slot)
                if (passes[p].cond == d.a[j].cond && (d.a[j].cond < 0 || passes[p].want == d.a[j].cond_want) &&
                    (counts || (passes[p].aw == w && passes[p].n < GBP_MAX_K)))
                    break;
            if (p == n_passes)
            {
                passes[n_passes].aw = counts ? 8 : w;
                passes[n_passes].cond = d.a[j].cond;
                passes[n_passes].want = d.a[j].cond_want;
                ++n_passes;
            }
            if (counts)
            {
                passes[p].counts |= 1u << j;
                continue;
            }
            passes[p].agg[passes[p].n++] = j;
            const int at = a->arg_types[j];
            passes[p].ext = passes[p].ext || at == CHGPU_I8 || at == CHGPU_I16 || at == CHGPU_I32 || at == CHGPU_F32;
        }
    if (n_passes == 0)
        n_passes = 1; // no function at all: one pass that only claims the groups

    const size_t key_w = chgpu_type_size(a->key_type);
    u32 cnt32 = 0;
    (void)agg_part_cell_bytes(a, a->key_type, n, &cnt32);
    // cells: four times the promised groups (4096 when nothing was promised), bounded by ~150 KiB of LDS; tables of up
    // to ~76 KiB let two 1024-thread workgroups share a CU
    const u32 s_dflt = (u32)chgpu_opt(ctx, "tune_agg_ranged_s", 4096);
    u32 S = s_dflt;
    if (a->size_hint)
        for (S = 1024; S < 4 * a->size_hint && S < lds_cells; S <<= 1)
            ;
    if (S > lds_cells)
        S = lds_cells;
    const size_t lds_ag = (size_t)PartLds(key_w <= 4 ? 4 : 8, S, a->words.n_words, cnt32).bytes() + 16;
    const u32 wg_per_cu = lds_ag <= 76 * 1024 ? 2 : 1;
    // flushes may claim up to grid * (S+1) cells above max fill: keep that inside the slack (capacity/2)
    const u64 max_grid = (a->t.capacity / 2) / (S + 1);
    u64 chunks = (u64)ctx->num_cus * wg_per_cu;
    if (chunks > max_grid)
        chunks = max_grid ? max_grid : 1;
    if (chunks > (n + 4095) / 4096)
        chunks = (n + 4095) / 4096;
    const u64 rows_per_chunk = ((n + chunks - 1) / chunks + 63) / 64 * 64;
    chunks = (n + rows_per_chunk - 1) / rows_per_chunk;
    const u8 * cond_ptr = filter ? (const u8 *)filter->data + row_begin : nullptr;
    if (chgpu_opt(ctx, "debug", 0))
    {
        std::string aw, ext, cnd; // per pass, comma-separated
        for (u32 p = 0; p < n_passes; ++p)
        {
            aw += (p ? "," : "") + std::to_string(passes[p].aw), ext += (p ? "," : "") + std::to_string(passes[p].ext ? 1 : 0);
            cnd += (p ? "," : "") + (passes[p].cond < 0 ? std::string("-") : std::to_string(passes[p].cond) + (passes[p].want ? "" : "!"));
        }
        fprintf(stderr, "chgpu: ranged GROUP BY n=%llu hint=%llu S=%u chunks=%llu passes=%u key_w=%zu aw=%s ext=%s%s%s\n", (unsigned long long)n,
                (unsigned long long)a->size_hint, S, (unsigned long long)chunks, n_passes, key_w, aw.c_str(), ext.c_str(), a->conditioned ? " conds=" : "",
                a->conditioned ? cnd.c_str() : "");
    }
    for (u32 p = 0; p < n_passes; ++p)
    {
        // this pass's descriptor: its argument functions, plus every count() in the first pass; state word indices are
        // the aggregator's own, so all passes meet in the same cells
        AggDesc dp = d;
        dp.n_aggs = 0;
        const void * rwords[GBP_MAX_K] = {nullptr, nullptr};
        for (u32 c = 0; c < passes[p].n; ++c)
        {
            const u32 j = passes[p].agg[c];
            dp.a[dp.n_aggs] = d.a[j];
            dp.a[dp.n_aggs].pre = c;
            ++dp.n_aggs;
            rwords[c] = (const char *)arg_cols[j]->data + row_begin * passes[p].aw;
        }
        for (u32 j = 0; j < a->n_aggs; ++j)
            if ((passes[p].counts >> j) & 1)
                dp.a[dp.n_aggs++] = d.a[j];
        const u8 * fcond_ptr = passes[p].cond >= 0 ? d.cond[passes[p].cond] + row_begin : nullptr;
        const u32 rk = passes[p].n;
        CHGPU_HIP(hipMemsetAsync(pending, 0, n_words64 * sizeof(u64), ctx->stream));
        int rc = CHGPU_OK;
        // keys of 1, 2, 4 or 8 bytes as the column holds them (KS), hashed as 4- or 8-byte keys (KT); arguments of 8, 4, 2 or 1 bytes,
        // sign- or float-extended where a narrow one needs it (EXT)
        dispatch_width(key_w, [&](auto ks) {
            using KS = decltype(ks);
            using KT = std::conditional_t<sizeof(KS) == 8, u64, u32>;
            dispatch_width(passes[p].aw, [&](auto at) {
                constexpr int AW = (int)sizeof(at);
                dispatch_const<0, 1>(AW < 8 && passes[p].ext ? 1 : 0, [&](auto x) { // (an 8-byte argument needs no extension)
                    constexpr bool EXT = decltype(x)::value != 0;
                    dispatch_const<0, 1>(fcond_ptr ? 1 : 0, [&](auto fc) {
                        constexpr bool FCOND = decltype(fc)::value != 0;
                        rc = launch_lds("ranged aggregation", k_agg_part_lds<KT, AW, KS, EXT, 0, FCOND>, dim3((u32)chunks), dim3(1024), lds_ag, ctx->stream, a->t, dp,
                                        (const KS *)key_col->data + row_begin, rwords[0], rwords[1], (const u64 *)nullptr, 1u, (u32)chunks, n, pending, S, rk, cnt32,
                                        rows_per_chunk, (const u32 *)nullptr, (u32 *)nullptr, cond_ptr, fcond_ptr, passes[p].want);
                    });
                });
            });
        });
        ctx->counters[6] += 1;
        CHGPU_TRY(rc);
        // rows this pass could not place (table at max fill) are retried with THIS pass's functions only
        CHGPU_TRY(agg_finish_rounds(a, dp, key_col->data, a->key_type, row_begin, n, pending));
    }
    return CHGPU_OK;
}

// The strategies that need no filtered copy of the block, chosen by promised / observed cardinality (see agg_add_block_impl).  The
// caller counts the rows.
static int agg_add_block_planned(chgpu_agg * a, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 n, const chgpu_col * filter,
                                 u32 lds_cells)
{
    chgpu_ctx * ctx = a->ctx;
    CHGPU_TRY(agg_fx_prepare_block(a, arg_cols, row_begin, n)); // (may widen the fixed-point window: before the descriptor is filled)
    AggDesc d;
    agg_fill_desc(a, arg_cols, &d);

    const u64 n_words64 = (n + 63) / 64;
    void * scratch = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, n_words64 * sizeof(u64) + 256, &scratch));
    u64 * pending = (u64 *)scratch;
    const u32 rows_grid = chgpu_grid_for(ctx, n, AGG_THREADS, 8);

    // Only the RANGE-mode arm applies `filter`: the caller sends a masked block here only when agg_takes_ranged says it ends there, and
    // every other arm refuses one instead of dropping its mask.
    const u64 lds_groups = (u64)lds_cells * 7 / 10;
    const bool tries_partitions = agg_tries_partitions(a, lds_groups, n);
    if (tries_partitions)
    {
        CHGPU_REQUIRE(!filter, CHGPU_ERR_LOGICAL, "a masked block reached the partitioned GROUP BY plans, which apply no mask");
        const int rc = agg_add_block_by_partitions(a, key_col, arg_cols, row_begin, n);
        if (rc != CHGPU_ERR_NOT_IMPLEMENTED)
            return rc;
    }
    CHGPU_TRY(agg_ensure_table(a, a->size_hint));
    if (agg_takes_ranged(a, lds_groups, n, tries_partitions))
        return agg_add_block_ranged(a, key_col, arg_cols, row_begin, n, filter, d, pending, n_words64, lds_cells);
    CHGPU_REQUIRE(!filter, CHGPU_ERR_LOGICAL, "a masked block reached the row-wise GROUP BY kernels, which apply no mask");
    // LDS-staged unless the caller promised a large cardinality (where nearly every key misses the LDS table)
    const bool use_lds = !a->has_extremum && a->size_hint <= 65536;
    if (chgpu_opt(ctx, "debug", 0))
        fprintf(stderr, "chgpu: direct GROUP BY n=%llu hint=%llu kernel=%s%s\n", (unsigned long long)n, (unsigned long long)a->size_hint, use_lds ? "rows_lds" : "rows_direct",
                a->conditioned ? " states=conditioned" : a->has_extremum ? " states=extremum" : "");
    if (use_lds)
    {
        // LDS cells per workgroup: the largest power of two with (1 + n_words) * 8 * (S+1) <= AGG_LDS_BYTES
        u32 S = 4096;
        while ((size_t)(S + 1) * 8 * (1 + a->words.n_words) > AGG_LDS_BYTES && S > 64)
            S >>= 1;
        // flushes may claim up to grid * (S+1) cells above max fill: keep that inside the slack (capacity/2)
        u64 max_grid = (a->t.capacity / 2) / (S + 1);
        const u32 lds_threads = (u32)chgpu_opt(ctx, "tune_agg_lds_threads", 512);
        u32 grid = chgpu_grid_for(ctx, n, lds_threads, lds_threads >= 1024 ? 2 : 4);
        if (grid > max_grid)
            grid = (u32)(max_grid ? max_grid : 1);
        const size_t lds = (size_t)(S + 1) * 8 * (1 + a->words.n_words);
        hipLaunchKernelGGL(k_agg_rows_lds, dim3(grid), dim3(lds_threads), lds, ctx->stream, a->t, d, key_col->data, a->key_type, row_begin, n, pending, S);
    }
    else
    {
        // one emplace + one atomic per state word and row
        d.row_seq = a->any_seq - row_begin; // any(): row i of the columns is the (any_seq + i - row_begin)-th row of the aggregation
        d.arg_sentinel = agg_arg_row_claim(a->any_seq + n);
        hipLaunchKernelGGL(k_agg_rows_direct<AGG_MODE_ALL>, dim3(rows_grid), dim3(AGG_THREADS), 0, ctx->stream, a->t, d, key_col->data, a->key_type, row_begin, n, pending);
    }
    ctx->counters[6] += 1;
    CHGPU_HIP(hipGetLastError());
    CHGPU_TRY(agg_finish_rounds(a, d, key_col->data, a->key_type, row_begin, n, pending));
    if (a->words.any)
    {
        hipLaunchKernelGGL(k_agg_any_resolve, dim3(rows_grid), dim3(AGG_THREADS), 0, ctx->stream, a->t, d, key_col->data, a->key_type, row_begin, n);
        ctx->counters[6] += 1;
        CHGPU_HIP(hipGetLastError());
    }
    if (a->words.arg)
    {
        // the claim and resolve passes, each behind a kernel boundary (the finish rounds left every row placed and every val key final)
        hipLaunchKernelGGL(k_agg_arg_rows<2>, dim3(rows_grid), dim3(AGG_THREADS), 0, ctx->stream, a->t, d, key_col->data, a->key_type, row_begin, n);
        hipLaunchKernelGGL(k_agg_arg_rows<3>, dim3(rows_grid), dim3(AGG_THREADS), 0, ctx->stream, a->t, d, key_col->data, a->key_type, row_begin, n);
        ctx->counters[6] += 2;
        CHGPU_HIP(hipGetLastError());
    }
    if (a->words.any || a->words.arg)
        a->any_seq += n;
    return CHGPU_OK;
}

static int agg_add_block_impl(chgpu_agg * a, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 row_end,
                              const chgpu_col * filter)
{
    CHGPU_REQUIRE(a, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(row_begin <= row_end, CHGPU_ERR_BAD_ARGUMENTS, "row_begin > row_end");
    a->started = true;
    chgpu_ctx * ctx = a->ctx;
    const u64 n = row_end - row_begin;
    if (filter)
    {
        CHGPU_REQUIRE(filter->type == CHGPU_U8, CHGPU_ERR_BAD_ARGUMENTS, "filter must be a UInt8 column");
        CHGPU_REQUIRE(row_end <= filter->rows, CHGPU_ERR_SIZES_MISMATCH, "filter has %llu rows, block ends at %llu",
                      (unsigned long long)filter->rows, (unsigned long long)row_end);
    }
    for (u32 j = 0; j < a->n_aggs; ++j)
        for (u32 sl = a->slot[j]; sl < agg_slot_end(a, j); ++sl)
        {
            const int want = sl == a->slot[j] ? a->arg_types[j] : a->val_types[j];
            CHGPU_REQUIRE(arg_cols && arg_cols[sl], CHGPU_ERR_BAD_ARGUMENTS, "argument column %u is NULL", sl);
            CHGPU_REQUIRE(arg_cols[sl]->type == want, CHGPU_ERR_BAD_ARGUMENTS, "argument column %u has type %d, expected %d", sl, arg_cols[sl]->type, want);
            CHGPU_REQUIRE(row_end <= arg_cols[sl]->rows, CHGPU_ERR_SIZES_MISMATCH, "argument column %u has %llu rows, block ends at %llu", sl,
                          (unsigned long long)arg_cols[sl]->rows, (unsigned long long)row_end);
        }
    if (a->key_type < 0)
        return agg_add_nokey(a, arg_cols, row_begin, row_end, filter);
    CHGPU_REQUIRE(key_col, CHGPU_ERR_BAD_ARGUMENTS, "key column is NULL");
    CHGPU_REQUIRE(key_col->type == a->key_type, CHGPU_ERR_BAD_ARGUMENTS, "key column has type %d, expected %d", key_col->type, a->key_type);
    CHGPU_REQUIRE(row_end <= key_col->rows, CHGPU_ERR_SIZES_MISMATCH, "key column has %llu rows, block ends at %llu",
                  (unsigned long long)key_col->rows, (unsigned long long)row_end);
    if (n == 0)
        return CHGPU_OK;
    if (a->t.find_only && a->n_aggs == 0)
        return CHGPU_OK; // SELECT k ... GROUP BY k with no_more_keys: nothing to find (Aggregator.cpp:1030-1034)
    // Strategy by promised/observed cardinality:
    //   groups <= what one workgroup's LDS table holds (~70 % of its cells)   -> LDS-staged (RANGE mode / k_agg_rows_lds)
    //   more, with enough rows to amortise two extra passes                   -> PARTITIONED
    //   otherwise (or hopelessly many groups)                                 -> DIRECT
    // Callers that gave no size hint (the reference adapts too: consecutive-key cache hit rate, Aggregator.cpp:944-958;
    // two-level conversion, :83-89): the first 1 Mi rows go through the LDS-staged kernel and the number of groups they
    // produced is extrapolated to the whole input.
    const u32 lds_cells = agg_part_max_cells(a->ctx, agg_part_cell_bytes(a, a->key_type, n, nullptr));
    const u64 lds_groups = (u64)lds_cells * 7 / 10;
    if (a->size_hint <= lds_groups && a->n_groups > lds_groups)
        a->size_hint = a->n_groups * 2; // the table already outgrew the LDS strategy
    if (a->size_hint == 0 && !a->hint_probed && n >= (8ull << 20) && !a->t.find_only) // (a find-only block adds no group: nothing to sample)
    {
        a->hint_probed = true;
        const u64 probe_rows = 1ull << 20;
        const u64 before = a->n_groups;
        CHGPU_TRY(agg_add_block_impl(a, key_col, arg_cols, row_begin, row_begin + probe_rows, filter));
        if (a->n_groups > lds_groups / 2)
        {
            const u64 est = agg_estimate_groups(a->n_groups - before, probe_rows);
            a->size_hint = before + est + est / 4;
        }
        return agg_add_block_impl(a, key_col, arg_cols, row_begin + probe_rows, row_end, filter);
    }
    // a WHERE mask is fused only into the RANGE-mode kernel; every other strategy gets the filtered block materialised first
    if (filter)
    {
        if (!agg_takes_ranged(a, lds_groups, n))
            return agg_add_block_materialised(a, key_col, arg_cols, row_begin, row_end, filter);
        // The aggregation kernel is issue-bound: it spends nearly the same time on a masked-out row as on a kept one, while
        // chgpu_filter_columns runs at HBM speed.  Measured break-even at ~30 % of the rows kept (1e9 rows, 1000 groups,
        // 10 % kept: 5.7 ms fused vs 5.3 ms materialised), so big blocks count the mask first (0.35 ms per 1e9 rows).
        if (n >= (16u << 20))
        {
            chgpu_col * fv = nullptr;
            CHGPU_TRY(chgpu_col_slice(ctx, filter, row_begin, n, &fv));
            u64 kept = 0;
            const int rc = chgpu_count_bytes_in_filter(ctx, fv, &kept);
            chgpu_col_free(fv);
            CHGPU_TRY(rc);
            if (kept == 0)
                return CHGPU_OK;
            if (kept * 10 < n * 3)
                return agg_add_block_materialised(a, key_col, arg_cols, row_begin, row_end, filter);
        }
    }
    CHGPU_TRY(agg_add_block_planned(a, key_col, arg_cols, row_begin, n, filter, lds_cells));
    ctx->counters[5] += n; // once per block, however many passes and calls the plan made over its rows
    return CHGPU_OK;
}

// merge tuples (keys + state word columns) with overflow handling
static int agg_merge_tuples(chgpu_agg * a, const u64 * src_keys, const u64 * src_words, u64 src_stride, u64 n, int skip_zero_keys, u64 zero_slot_index)
{
    chgpu_ctx * ctx = a->ctx;
    if (n == 0)
        return CHGPU_OK;
    CHGPU_TRY(agg_ensure_table(a, a->size_hint));
    const u64 n_words64 = (n + 63) / 64;
    void * scratch = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, n_words64 * sizeof(u64) + 256, &scratch));
    u64 * pending = (u64 *)scratch;
    const u32 grid = chgpu_grid_for(ctx, n, AGG_THREADS, 8);
    hipLaunchKernelGGL(k_agg_tuples<AGG_MODE_ALL>, dim3(grid), dim3(AGG_THREADS), 0, ctx->stream, a->t, AggMergeWords(a->words), 0u, src_keys, src_words, src_stride, n, skip_zero_keys, zero_slot_index, 1, pending);
    ctx->counters[6] += 1;
    CHGPU_HIP(hipGetLastError());
    for (int round = 0; round < 64; ++round)
    {
        AggCtrl c;
        CHGPU_TRY(agg_read_ctrl(a, &c));
        if (!c.overflow)
        {
            if (a->words.arg)
            {
                // argMin / argMax: every val key is final; the source states that hold one claim, then the winner stores its arg
                hipLaunchKernelGGL(k_agg_arg_tuples<2>, dim3(grid), dim3(AGG_THREADS), 0, ctx->stream, a->t, a->words, src_keys, src_words, src_stride, n,
                                   skip_zero_keys, zero_slot_index);
                hipLaunchKernelGGL(k_agg_arg_tuples<3>, dim3(grid), dim3(AGG_THREADS), 0, ctx->stream, a->t, a->words, src_keys, src_words, src_stride, n,
                                   skip_zero_keys, zero_slot_index);
                ctx->counters[6] += 2;
                CHGPU_HIP(hipGetLastError());
            }
            return CHGPU_OK;
        }
        CHGPU_TRY(agg_grow(a, c.n_groups, c.has_zero != 0));
        hipLaunchKernelGGL(k_agg_tuples<AGG_MODE_PENDING>, dim3(grid), dim3(AGG_THREADS), 0, ctx->stream, a->t, AggMergeWords(a->words), 0u, src_keys, src_words, src_stride, n, skip_zero_keys, zero_slot_index, 1, pending);
        ctx->counters[6] += 1;
        CHGPU_HIP(hipGetLastError());
    }
    return chgpu_set_error(CHGPU_ERR_LOGICAL, "aggregation merge did not converge after 64 growth rounds");
}

// One state row `src` folded into the row `dst` of the same layout, on the host (mergeWithoutKeyDataImpl, Aggregator.cpp:2584-2628):
// the states of an aggregation without key, an overflow row
static void agg_combine_row(const AggWords & ws, u64 * dst, const u64 * src)
{
    for (u32 w = 0; w < ws.n_words; ++w)
    {
        if ((ws.fx_high >> w) & 1)
            continue; // with its low half
        if ((ws.fx >> w) & 1)
        {
            const u32 h = ws.fx_hi[w];
            const u64 lo = dst[w] + src[w];
            dst[h] += src[h] + (lo < dst[w] ? 1 : 0);
            dst[w] = lo;
        }
        else if ((ws.any >> w) & 1)
        {
            if (dst[w] == 0 && src[w] != 0) // changeFirstTime: a state that has a value keeps it
                dst[w] = src[w], dst[w + 1] = src[w + 1];
            ++w;
        }
        else if ((ws.arg >> w) & 1)
        {
            // a source that has a value replaces a state without one, or one whose val is strictly worse; {val, arg} move together and
            // the claim becomes ~0: older than every row to come
            if (src[w + 1] != 0 && (dst[w + 1] == 0 || src[w] > dst[w]))
                dst[w] = src[w], dst[w + 1] = ~0ull, dst[w + 2] = src[w + 2];
            w += 2;
        }
        else if (ws.op(w) == 2)
            dst[w] = src[w] > dst[w] ? src[w] : dst[w]; // min / max order keys
        else if (ws.op(w) == 1)
        {
            double x, y;
            memcpy(&x, &dst[w], 8);
            memcpy(&y, &src[w], 8);
            x += y;
            memcpy(&dst[w], &x, 8);
        }
        else
            dst[w] += src[w];
    }
}

static bool agg_same_shape(const chgpu_agg * x, const chgpu_agg * y)
{
    if (x->key_type != y->key_type || x->n_aggs != y->n_aggs)
        return false;
    for (u32 j = 0; j < x->n_aggs; ++j)
        if (x->kinds[j] != y->kinds[j] || x->arg_types[j] != y->arg_types[j] || x->cond_modes[j] != y->cond_modes[j])
            return false;
    return true;
}

// Both sides of a merge to ONE fixed-point window (see chgpu_agg_merge)
static int agg_merge_align_fx(chgpu_agg * dst, const chgpu_agg * src)
{
    if (dst->words.fx || src->words.fx)
    {
        // fixed-point sums: both sides to ONE window first (the source's states are re-expressed in place: same values, possibly a coarser
        // unit -- the reference's merge consumes its source too), or both back to doubles when one of them met a NaN / infinity
        chgpu_agg * s = const_cast<chgpu_agg *>(src);
        if (!dst->words.fx || !s->words.fx)
        {
            CHGPU_TRY(agg_fx_to_plain(dst));
            CHGPU_TRY(agg_fx_to_plain(s));
        }
        else if (s->fx_base_set)
        {
            if (!dst->fx_base_set)
            {
                CHGPU_TRY(agg_fx_set_window(dst, s->fx_base, s->fx_log_cap));
                dst->fx_rows += s->fx_rows;
                dst->fx_emin = s->fx_emin;
            }
            else
            {
                int log_cap = dst->fx_log_cap > s->fx_log_cap ? dst->fx_log_cap : s->fx_log_cap;
                const u64 rows = dst->fx_rows + s->fx_rows;
                while (log_cap < 62 && rows > (1ull << log_cap))
                    log_cap += 8;
                const int bd = dst->fx_base + (log_cap - dst->fx_log_cap), bs = s->fx_base + (log_cap - s->fx_log_cap);
                const int base = bd > bs ? bd : bs;
                const int emin = dst->fx_emin < s->fx_emin ? dst->fx_emin : s->fx_emin;
                if (emin + 1 - FX_MIN_BITS < base)
                {
                    CHGPU_TRY(agg_fx_to_plain(dst));
                    CHGPU_TRY(agg_fx_to_plain(s));
                }
                else
                {
                    CHGPU_TRY(agg_fx_set_window(dst, base, log_cap));
                    CHGPU_TRY(agg_fx_set_window(s, base, log_cap));
                    dst->fx_emin = emin;
                    dst->fx_rows = rows;
                }
            }
        }
        if (src->ctx != dst->ctx)
            CHGPU_HIP(hipStreamSynchronize(src->ctx->stream)); // (the re-expression ran on the source's stream)
    }
    return CHGPU_OK;
}

// The overflow rows merge like states without key: src's words (host copy, the window already shared) folded into dst's, on the host
// -- one row of at most AGG_MAX_WORDS words
static int agg_fold_overflow_words(chgpu_agg * dst, const u64 * in)
{
    if (!dst->ovf_mem)
    {
        CHGPU_TRY(chgpu_pool_alloc(dst->ctx, AGG_MAX_WORDS * 8, &dst->ovf_mem, &dst->ovf_class));
        CHGPU_HIP(hipMemsetAsync(dst->ovf_mem, 0, AGG_MAX_WORDS * 8, dst->ctx->stream));
    }
    u64 o[AGG_MAX_WORDS] = {0};
    CHGPU_TRY(chgpu_read_back(dst->ctx, dst->ovf_mem, o, dst->words.n_words * 8));
    agg_combine_row(dst->words, o, in);
    CHGPU_HIP(hipMemcpyAsync(dst->ovf_mem, o, dst->words.n_words * 8, hipMemcpyHostToDevice, dst->ctx->stream));
    CHGPU_HIP(hipStreamSynchronize(dst->ctx->stream)); // (o is on this stack frame)
    return CHGPU_OK;
}
static int agg_merge_overflow_rows(chgpu_agg * dst, const chgpu_agg * src)
{
    if (!src->ovf_mem)
        return CHGPU_OK;
    u64 in[AGG_MAX_WORDS] = {0};
    CHGPU_TRY(chgpu_read_back(src->ctx, src->ovf_mem, in, src->words.n_words * 8));
    return agg_fold_overflow_words(dst, in);
}

extern "C" int chgpu_agg_merge(chgpu_agg * dst, const chgpu_agg * src)
{
    ChgpuDeviceGuard _dev_guard(dst ? dst->ctx : nullptr);
    CHGPU_REQUIRE(dst && src, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(agg_same_shape(dst, src), CHGPU_ERR_BAD_ARGUMENTS, "cannot merge aggregation states of different shape");
    // variants of different pipeline streams live on different contexts: the source's kernels run on ITS stream and must have finished
    // before this context's stream reads its table (the reference merges after every stream has finished consuming)
    if (src->ctx != dst->ctx)
        CHGPU_HIP(hipStreamSynchronize(src->ctx->stream));
    if (dst->key_type < 0)
    {
        // mergeWithoutKeyDataImpl (Aggregator.cpp:2584-2628)
        agg_combine_row(dst->words, dst->host_words, src->host_words);
        dst->nokey_kept += src->nokey_kept;
        return CHGPU_OK;
    }
    if (!src->table_mem && !src->ovf_mem)
        return CHGPU_OK;
    CHGPU_REQUIRE(dst->words.n_words == src->words.n_words, CHGPU_ERR_BAD_ARGUMENTS, "cannot merge aggregations created under different deterministic_float_sums settings");
    CHGPU_TRY(agg_merge_align_fx(dst, src));
    CHGPU_TRY(agg_merge_overflow_rows(dst, src));
    if (!src->table_mem)
        return CHGPU_OK;
    // the source's zero cell participates only when it is set
    AggCtrl sc;
    CHGPU_TRY(chgpu_read_back(dst->ctx, src->t.ctrl, &sc, sizeof(sc)));
    const u64 n = src->t.capacity + (sc.has_zero ? 1 : 0);
    return agg_merge_tuples(dst, src->t.keys, src->t.words, src->t.capacity + 1, n, 1, sc.has_zero ? src->t.capacity : ~0ull);
}

// The public state columns a merge is given: one per public word, 8 bytes wide, `rows` rows at least.  (An is_overflows block answers
// a narrow or short column with one message of its own.)
static int agg_check_state_cols(const chgpu_agg * dst, const chgpu_col * const * state_cols, u64 rows, bool is_overflows)
{
    for (u32 w = 0; w < dst->words.n_pub_words; ++w)
    {
        CHGPU_REQUIRE(state_cols[w], CHGPU_ERR_BAD_ARGUMENTS, "state column %u is NULL", w);
        const bool wide = chgpu_type_size(state_cols[w]->type) == 8, tall = state_cols[w]->rows >= rows;
        if (is_overflows)
            CHGPU_REQUIRE(wide && tall, CHGPU_ERR_BAD_ARGUMENTS, "state column %u: 8-byte words, %llu rows", w, (unsigned long long)rows);
        else
        {
            CHGPU_REQUIRE(wide, CHGPU_ERR_BAD_ARGUMENTS, "state column %u must be 8 bytes wide", w);
            CHGPU_REQUIRE(tall, CHGPU_ERR_SIZES_MISMATCH, "state column %u shorter than %llu rows", w, (unsigned long long)rows);
        }
    }
    return CHGPU_OK;
}

// Float64 sum states arriving in state columns for fixed-point sums: each of the `rows` states is one value for the window -- or, with
// a NaN / infinity among them, the end of the fixed-point mode (agg_fx_to_plain)
static int agg_fx_admit_states(chgpu_agg * dst, const chgpu_col * const * state_cols, u64 rows)
{
    if (!dst->words.fx)
        return CHGPU_OK;
    u32 emax = 0, emin = 2047;
    for (u32 w = 0; w < dst->words.n_pub_words; ++w)
        if ((dst->words.fx >> w) & 1)
        {
            u32 e = 0, em = 2047;
            bool bad = false;
            CHGPU_TRY(agg_fx_stats(dst->ctx, state_cols[w]->data, CHGPU_F64, 0, rows, nullptr, 0, &e, &em, &bad));
            if (bad)
                return agg_fx_to_plain(dst);
            emax = e > emax ? e : emax;
            emin = em < emin ? em : emin;
        }
    return agg_fx_admit(dst, emax, emin, rows);
}

extern "C" int chgpu_agg_merge_states(chgpu_agg * dst, const chgpu_col * key_col, const chgpu_col * const * state_cols, uint64_t rows)
{
    ChgpuDeviceGuard _dev_guard(dst ? dst->ctx : nullptr);
    CHGPU_REQUIRE(dst && state_cols, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    chgpu_ctx * ctx = dst->ctx;
    CHGPU_TRY(agg_check_state_cols(dst, state_cols, rows, false));
    if (dst->key_type < 0)
    {
        CHGPU_REQUIRE(rows <= 1, CHGPU_ERR_BAD_ARGUMENTS, "without_key states merge one row at a time");
        if (rows == 0)
            return CHGPU_OK;
        u64 in[AGG_MAX_WORDS] = {0};
        for (u32 w = 0; w < dst->words.n_words; ++w)
            CHGPU_TRY(chgpu_read_back(ctx, state_cols[w]->data, &in[w], 8));
        bool any_set = false;
        for (u32 w = 0; w < dst->words.n_words; ++w)
            any_set = any_set || in[w] != 0;
        agg_combine_row(dst->words, dst->host_words, in);
        dst->nokey_kept += any_set ? 1 : 0; // (a partial state of an empty input is all zeros)
        return CHGPU_OK;
    }
    CHGPU_REQUIRE(key_col && key_col->rows >= rows, CHGPU_ERR_SIZES_MISMATCH, "key column shorter than %llu rows", (unsigned long long)rows);
    CHGPU_REQUIRE(key_col->type == dst->key_type, CHGPU_ERR_BAD_ARGUMENTS, "key column type mismatch");
    if (rows == 0)
        return CHGPU_OK;
    CHGPU_TRY(agg_fx_admit_states(dst, state_cols, rows));
    // stage into one SoA buffer [keys u64][words...] so the tuple kernel sees a single stride
    chgpu_col * stage = nullptr;
    CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, rows * (1 + dst->words.n_words), &stage));
    u64 * sk = (u64 *)stage->data;
    int rc = CHGPU_OK;
    {
        const u32 grid = chgpu_grid_for(ctx, rows, 256, 8);
        // widen keys with the same zero-extension as the row path (reuse k_narrow in reverse via a tiny lambda kernel)
        switch (chgpu_type_size(key_col->type))
        {
            case 8: rc = hipMemcpyAsync(sk, key_col->data, rows * 8, hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess ? CHGPU_OK : CHGPU_ERR_DEVICE; break;
            default:
            {
                extern __global__ void k_widen_keys(const void *, int, u64, u64 *);
                hipLaunchKernelGGL(k_widen_keys, dim3(grid), dim3(256), 0, ctx->stream, (const void *)key_col->data, key_col->type, (u64)rows, sk);
                break;
            }
        }
        for (u32 w = 0; w < dst->words.n_pub_words && rc == CHGPU_OK; ++w)
        {
            if ((dst->words.fx >> w) & 1)
            {
                hipLaunchKernelGGL(k_fx_from_double, dim3(grid), dim3(256), 0, ctx->stream, (const u64 *)state_cols[w]->data, (u64)rows, dst->fx_base,
                                   sk + (u64)(w + 1) * rows, sk + (u64)(dst->words.fx_hi[w] + 1) * rows);
                ctx->counters[6] += 1;
                continue;
            }
            rc = hipMemcpyAsync(sk + (u64)(w + 1) * rows, state_cols[w]->data, rows * 8, hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess ? CHGPU_OK : CHGPU_ERR_DEVICE;
        }
    }
    if (rc == CHGPU_OK)
        rc = agg_merge_tuples(dst, sk, sk + rows, rows, rows, 0, ~0ull);
    else
        chgpu_set_error(CHGPU_ERR_DEVICE, "staging copy failed");
    chgpu_col_free(stage);
    return rc;
}

// ---- max_rows_to_group_by / group_by_overflow_mode / overflow_row ----
extern "C" int chgpu_agg_set_limits(chgpu_agg * a, uint64_t max_rows_to_group_by, int group_by_overflow_mode, int overflow_row)
{
    CHGPU_REQUIRE(a, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(group_by_overflow_mode >= CHGPU_OVERFLOW_THROW && group_by_overflow_mode <= CHGPU_OVERFLOW_ANY, CHGPU_ERR_BAD_ARGUMENTS,
                  "unknown group_by_overflow_mode %d", group_by_overflow_mode);
    CHGPU_REQUIRE(!a->started, CHGPU_ERR_BAD_ARGUMENTS, "GROUP BY limits must be set before the first block");
    a->max_rows = max_rows_to_group_by;
    a->overflow_mode = group_by_overflow_mode;
    a->overflow_row = overflow_row != 0;
    return CHGPU_OK;
}

// Aggregator::checkLimits (Aggregator.cpp:1816-1830) on `groups` (zero key included, overflow row excluded): THROW fails, BREAK clears
// *keep, ANY sets *no_more_keys
static int agg_check_limits(chgpu_agg * a, u64 groups, int * no_more_keys, int * keep)
{
    if (a->max_rows == 0 || groups <= a->max_rows)
        return CHGPU_OK;
    switch (a->overflow_mode)
    {
        case CHGPU_OVERFLOW_THROW:
            return chgpu_set_error(CHGPU_ERR_TOO_MANY_ROWS, "Limit for rows to GROUP BY exceeded: has %llu rows, maximum: %llu", (unsigned long long)groups,
                                   (unsigned long long)a->max_rows);
        case CHGPU_OVERFLOW_BREAK: *keep = 0; break;
        default: *no_more_keys = 1; break;
    }
    return CHGPU_OK;
}

static int agg_execute_limited(chgpu_agg * a, const chgpu_col * key_col, const chgpu_col * const * arg_cols, u64 row_begin, u64 row_end,
                               const chgpu_col * filter_u8, int * no_more_keys, int * keep_reading)
{
    *keep_reading = 1;
    if (a->key_type < 0)
        return agg_add_block_impl(a, key_col, arg_cols, row_begin, row_end, filter_u8); // without key: limits never trigger
    CHGPU_TRY(agg_ensure_overflow_row(a));
    const bool find_only = *no_more_keys != 0;
    agg_set_find_only(a, find_only);
    const int rc = agg_add_block_impl(a, key_col, arg_cols, row_begin, row_end, filter_u8);
    agg_set_find_only(a, false);
    CHGPU_TRY(rc);
    if (find_only || a->max_rows == 0)
        return CHGPU_OK;
    // every plan ends on a read-back of the table's header (agg_finish_rounds*): a->n_groups is this block's result; a table that does
    // not exist yet holds no group
    return agg_check_limits(a, a->table_mem ? a->n_groups : 0, no_more_keys, keep_reading);
}

extern "C" int chgpu_agg_execute_on_block(chgpu_agg * a, const chgpu_col * key_col, const chgpu_col * const * arg_cols, uint64_t row_begin,
                                          uint64_t row_end, const chgpu_col * filter_u8, int * no_more_keys, int * keep_reading)
{
    ChgpuDeviceGuard _dev_guard(a ? a->ctx : nullptr);
    CHGPU_REQUIRE(a && no_more_keys && keep_reading, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    AGG_REQUIRE_UNCONDITIONED(a);
    return agg_execute_limited(a, key_col, arg_cols, row_begin, row_end, filter_u8, no_more_keys, keep_reading);
}

extern "C" int chgpu_agg_execute_on_block_conditional(chgpu_agg * a, const chgpu_col * key_col, const chgpu_col * const * arg_cols,
                                                      const chgpu_col * const * cond_cols, uint64_t row_begin, uint64_t row_end,
                                                      const chgpu_col * filter_u8, int * no_more_keys, int * keep_reading)
{
    ChgpuDeviceGuard _dev_guard(a ? a->ctx : nullptr);
    CHGPU_REQUIRE(a, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE((no_more_keys == nullptr) == (keep_reading == nullptr), CHGPU_ERR_BAD_ARGUMENTS, "no_more_keys and keep_reading go together");
    for (u32 j = 0; a->conditioned && j < a->n_aggs; ++j)
    {
        if (a->cond_modes[j] == CHGPU_AGG_COND_NONE)
            continue;
        CHGPU_REQUIRE(cond_cols && cond_cols[j], CHGPU_ERR_BAD_ARGUMENTS, "condition column of function %u is NULL", j);
        CHGPU_REQUIRE(cond_cols[j]->type == CHGPU_U8, CHGPU_ERR_BAD_ARGUMENTS, "condition column of function %u must be a UInt8 column", j);
        CHGPU_REQUIRE(row_end <= cond_cols[j]->rows, CHGPU_ERR_SIZES_MISMATCH, "condition column of function %u has %llu rows, block ends at %llu", j,
                      (unsigned long long)cond_cols[j]->rows, (unsigned long long)row_end);
    }
    a->block_conds = a->conditioned ? cond_cols : nullptr;
    const int rc = no_more_keys ? agg_execute_limited(a, key_col, arg_cols, row_begin, row_end, filter_u8, no_more_keys, keep_reading)
                                : agg_add_block_impl(a, key_col, arg_cols, row_begin, row_end, filter_u8);
    a->block_conds = nullptr;
    return rc;
}

extern "C" int chgpu_agg_merge_limited(chgpu_agg * dst, const chgpu_agg * src, int * no_more_keys, int * keep_merging)
{
    ChgpuDeviceGuard _dev_guard(dst ? dst->ctx : nullptr);
    CHGPU_REQUIRE(dst && src && no_more_keys && keep_merging, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    *keep_merging = 1;
    if (dst->key_type < 0)
        return chgpu_agg_merge(dst, src);
    CHGPU_REQUIRE(agg_same_shape(dst, src) && dst->words.n_words == src->words.n_words, CHGPU_ERR_BAD_ARGUMENTS, "cannot merge aggregation states of different shape");
    dst->started = true;
    // mergeSingleLevelDataImpl: checkLimits on dst's size before the source is merged
    if (!*no_more_keys)
    {
        u64 g = 0;
        CHGPU_TRY(chgpu_agg_size(dst, &g));
        CHGPU_TRY(agg_check_limits(dst, g, no_more_keys, keep_merging));
    }
    if (!*keep_merging)
    {
        // BREAK: no more keyed data; the overflow rows still merge (mergeWithoutKeyDataImpl)
        if (src->ctx != dst->ctx)
            CHGPU_HIP(hipStreamSynchronize(src->ctx->stream));
        if (!src->ovf_mem)
            return CHGPU_OK;
        CHGPU_TRY(agg_merge_align_fx(dst, src));
        return agg_merge_overflow_rows(dst, src);
    }
    if (!*no_more_keys)
        return chgpu_agg_merge(dst, src);
    // mergeDataNoMoreKeysImpl / mergeDataOnlyExistingKeysImpl: find-only, a missing key's state to dst's overflow row or dropped
    CHGPU_TRY(agg_ensure_overflow_row(dst));
    agg_set_find_only(dst, true);
    const int rc = chgpu_agg_merge(dst, src);
    agg_set_find_only(dst, false);
    return rc;
}

extern "C" int chgpu_agg_merge_states_limited(chgpu_agg * dst, const chgpu_col * key_col, const chgpu_col * const * state_cols, uint64_t rows,
                                              int is_overflows, int * no_more_keys, int * keep_reading)
{
    ChgpuDeviceGuard _dev_guard(dst ? dst->ctx : nullptr);
    CHGPU_REQUIRE(dst && state_cols && no_more_keys && keep_reading, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    *keep_reading = 1;
    if (dst->key_type < 0)
        return chgpu_agg_merge_states(dst, key_col, state_cols, rows);
    dst->started = true;
    if (is_overflows)
    {
        // a block flagged is_overflows: its (one) row merges into the overflow row (mergeBlockWithoutKeyStreamsImpl)
        CHGPU_REQUIRE(rows <= 1, CHGPU_ERR_BAD_ARGUMENTS, "an is_overflows block has one row");
        CHGPU_TRY(agg_check_state_cols(dst, state_cols, rows, true));
        if (rows == 0)
            return CHGPU_OK;
        u64 in[AGG_MAX_WORDS] = {0};
        for (u32 w = 0; w < dst->words.n_pub_words; ++w)
            CHGPU_TRY(chgpu_read_back(dst->ctx, state_cols[w]->data, &in[w], 8));
        // Float64 states of fixed-point sums: admitted to the window like any state column, then converted
        CHGPU_TRY(agg_fx_admit_states(dst, state_cols, 1));
        for (u32 w = 0; w < dst->words.n_pub_words; ++w)
            if ((dst->words.fx >> w) & 1)
            {
                const Fx128 x = fx_from_double(in[w], dst->fx_base);
                in[w] = x.lo, in[dst->words.fx_hi[w]] = x.hi;
            }
        return agg_fold_overflow_words(dst, in);
    }
    const bool find_only = *no_more_keys != 0;
    if (find_only)
        CHGPU_TRY(agg_ensure_overflow_row(dst));
    agg_set_find_only(dst, find_only);
    const int rc = chgpu_agg_merge_states(dst, key_col, state_cols, rows);
    agg_set_find_only(dst, false);
    CHGPU_TRY(rc);
    // mergeOnBlock checks the limits after the block, as executeOnBlock does
    if (find_only || dst->max_rows == 0)
        return CHGPU_OK;
    u64 g = 0;
    CHGPU_TRY(chgpu_agg_size(dst, &g));
    return agg_check_limits(dst, g, no_more_keys, keep_reading);
}

// The state word that tells whether any row reached function j (0 = none): its `seen` word, avg's denominator, the claim of any /
// argMin / argMax; ~0 = it has none (count; an -If sum, whose empty state already reads 0; an unconditioned min / max)
static u32 agg_reached_word(const chgpu_agg * a, u32 j)
{
    const AggKind & k = agg_kind(a->kinds[j]);
    const u32 rw = a->word_off[j] + k.reached;
    return k.reached < k.words || ((a->words.seen >> rw) & 1) ? rw : ~0u;
}
// The overflow row: final -> one result per aggregate (the without-key conventions: count / sum 0, avg NaN, min / max / any the type's
// default when no row reached it), else its raw state words as chgpu_agg_export_states gives them.  One-row columns; *has = 0 when the
// aggregation has none.
extern "C" int chgpu_agg_overflow_row(chgpu_agg * a, int final, chgpu_col ** cols, int * has)
{
    ChgpuDeviceGuard _dev_guard(a ? a->ctx : nullptr);
    CHGPU_REQUIRE(a && cols && has, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    *has = 0;
    if (a->key_type < 0 || !a->ovf_mem)
        return CHGPU_OK;
    chgpu_ctx * ctx = a->ctx;
    u64 o[AGG_MAX_WORDS] = {0};
    CHGPU_TRY(chgpu_read_back(ctx, a->ovf_mem, o, a->words.n_words * 8));
    // fixed-point pairs to their Float64 value (the public word)
    u64 pub[AGG_MAX_WORDS] = {0};
    for (u32 w = 0; w < a->words.n_pub_words; ++w)
    {
        pub[w] = o[w];
        if ((a->words.fx >> w) & 1)
        {
            const double x = fx_to_double(o[w], o[a->words.fx_hi[w]], a->fx_base);
            memcpy(&pub[w], &x, 8);
        }
    }
    const u32 n_out = final ? a->n_aggs : a->words.n_pub_words;
    for (u32 k = 0; k < n_out; ++k)
        cols[k] = nullptr;
    int rc = CHGPU_OK;
    if (!final)
    {
        for (u32 w = 0; w < a->words.n_pub_words && rc == CHGPU_OK; ++w)
            rc = chgpu_col_upload(ctx, a->words.pub_type(w), &pub[w], 1, &cols[w]);
    }
    else
        for (u32 j = 0; j < a->n_aggs && rc == CHGPU_OK; ++j)
        {
            const u32 w = a->word_off[j];
            const AggKind & k = agg_kind(a->kinds[j]);
            const int at = a->arg_types[j];
            const bool f = chgpu_type_is_float(at);
            u64 v = 0;
            int type = CHGPU_U64;
            switch (a->kinds[j])
            {
                case CHGPU_AGG_COUNT: v = pub[w]; break;
                case CHGPU_AGG_SUM: v = pub[w], type = chgpu_sum_result_type(at); break;
                case CHGPU_AGG_AVG:
                {
                    double num;
                    if (f)
                        memcpy(&num, &pub[w], 8);
                    else
                        num = chgpu_sum_result_type(at) == CHGPU_I64 ? (double)(i64)pub[w] : (double)pub[w];
                    double r = num / (double)pub[w + 1]; // 0 / 0 = NaN, as without key
                    if (a->cond_modes[j] == CHGPU_AGG_COND_NULL && pub[w + 1] == 0)
                        r = 0.0; // the nested default of a NULL result
                    memcpy(&v, &r, 8);
                    type = CHGPU_F64;
                    break;
                }
                default:
                {
                    // min / max / any / argMin / argMax: the value in the argument's type; the type's default when no row reached it
                    // a row reached it: a conditioned min / max has its `seen` word, any / argMin / argMax their claim; a bare min / max
                    // key is non-zero once set
                    type = at;
                    const u32 rw = agg_reached_word(a, j);
                    const bool reached = pub[rw == ~0u ? w : rw] != 0;
                    if (reached)
                        v = k.words > 1 ? pub[w + k.result] : agg_order_key_inverse(a->kinds[j] == CHGPU_AGG_MIN ? ~pub[w] : pub[w], at); // (any, arg: bits as loaded)
                    if (at == CHGPU_F32)
                    {
                        double x;
                        memcpy(&x, &v, 8);
                        const float y = (float)x; // (the widening was exact: so is this)
                        v = 0;
                        memcpy(&v, &y, 4);
                    }
                    break;
                }
            }
            rc = chgpu_col_upload(ctx, type, &v, 1, &cols[j]); // (little endian: a narrower type takes the low bytes)
        }
    if (rc != CHGPU_OK)
    {
        for (u32 k = 0; k < n_out; ++k)
            if (cols[k])
                chgpu_col_free(cols[k]), cols[k] = nullptr;
        return rc;
    }
    *has = 1;
    return CHGPU_OK;
}

__global__ __launch_bounds__(256) void k_widen_keys(const void * keys, int type, u64 n, u64 * out)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
        out[i] = load_key_zext(keys, type, i);
}

extern "C" int chgpu_agg_size(chgpu_agg * a, uint64_t * groups)
{
    ChgpuDeviceGuard _dev_guard(a ? a->ctx : nullptr);
    CHGPU_REQUIRE(a && groups, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    if (a->key_type < 0)
    {
        *groups = 1; // no-key aggregation always yields one row (AggregatingTransform.cpp:700-708)
        return CHGPU_OK;
    }
    if (!a->table_mem)
    {
        *groups = 0;
        return CHGPU_OK;
    }
    AggCtrl c;
    CHGPU_TRY(agg_read_ctrl(a, &c));
    *groups = c.n_groups;
    return CHGPU_OK;
}

// keys + raw state words compacted out of the table (table order; the reference's order is unspecified too)
static int agg_export(chgpu_agg * a, chgpu_col ** keys_out, chgpu_col ** word_cols /* [n_words] */, u64 * groups)
{
    chgpu_ctx * ctx = a->ctx;
    for (u32 w = 0; w < a->words.n_words; ++w)
        word_cols[w] = nullptr;
    if (a->key_type < 0)
    {
        for (u32 w = 0; w < a->words.n_words; ++w)
        {
            CHGPU_TRY(chgpu_col_upload(ctx, a->words.pub_type(w), &a->host_words[w], 1, &word_cols[w]));
        }
        if (keys_out)
            *keys_out = nullptr;
        *groups = 1;
        return CHGPU_OK;
    }
    if (!a->table_mem)
    {
        if (keys_out)
            CHGPU_TRY(chgpu_col_new(ctx, a->key_type, 0, keys_out));
        for (u32 w = 0; w < a->words.n_pub_words; ++w)
            CHGPU_TRY(chgpu_col_new(ctx, a->words.pub_type(w), 0, &word_cols[w]));
        *groups = 0;
        return CHGPU_OK;
    }
    const u64 cells = a->t.capacity + 1;
    chgpu_col * mask = nullptr;
    CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U8, cells, &mask));
    const u32 grid = chgpu_grid_for(ctx, cells, 256, 8);
    hipLaunchKernelGGL(k_fix_zero_key, dim3(1), dim3(64), 0, ctx->stream, a->t.keys, a->t.capacity);
    hipLaunchKernelGGL(k_occupied_mask, dim3(grid), dim3(256), 0, ctx->stream, a->t.keys, a->t.capacity, a->t.ctrl, (u8 *)mask->data);
    ctx->counters[6] += 2;
    int rc = CHGPU_OK;
    u64 n_out = 0;
    chgpu_col view;
    view.ctx = ctx;
    view.rows = cells;
    view.owns = false;
    // keys and every state word in ONE filter call: one count + scan + read-back instead of one per column (all 8-byte columns: they share
    // a compaction kernel)
    chgpu_col * k64 = nullptr;
    {
        chgpu_col views[1 + AGG_MAX_WORDS];
        const chgpu_col * vin[1 + AGG_MAX_WORDS];
        chgpu_col * vout[1 + AGG_MAX_WORDS] = {nullptr};
        for (u32 c = 0; c <= a->words.n_words; ++c)
        {
            views[c] = view;
            views[c].type = c == 0 || a->words.op(c - 1) != 1 ? CHGPU_U64 : CHGPU_F64; // (a fixed-point pair: two integer words until it is folded below)
            views[c].data = c == 0 ? (void *)a->t.keys : (void *)(a->t.words + (u64)(c - 1) * cells);
            vin[c] = &views[c];
        }
        rc = chgpu_filter_columns(ctx, 1 + a->words.n_words, vin, mask, 0, vout, &n_out);
        if (rc == CHGPU_OK)
        {
            k64 = vout[0];
            for (u32 w = 0; w < a->words.n_words; ++w)
                word_cols[w] = vout[1 + w];
        }
    }
    chgpu_col_free(mask);
    auto drop_words = [&]() {
        for (u32 w = 0; w < a->words.n_words; ++w)
        {
            chgpu_col_free(word_cols[w]); // the word columns already filtered when a later step failed
            word_cols[w] = nullptr;
        }
    };
    if (rc == CHGPU_OK)
    {
        // the fixed-point sums leave as the doubles they stand for (one rounding per group); the spare high words stay inside
        for (u32 w = 0; w < a->words.n_pub_words; ++w)
            if ((a->words.fx >> w) & 1)
            {
                if (n_out)
                {
                    hipLaunchKernelGGL(k_fx_to_double, dim3(chgpu_grid_for(ctx, n_out, 256, 8)), dim3(256), 0, ctx->stream, (u64 *)word_cols[w]->data,
                                       (u64 *)word_cols[a->words.fx_hi[w]]->data, n_out, a->fx_base, 0);
                    ctx->counters[6] += 1;
                }
                word_cols[w]->type = CHGPU_F64;
            }
        for (u32 w = a->words.n_pub_words; w < a->words.n_words; ++w)
        {
            chgpu_col_free(word_cols[w]); // pooled: reuse is stream-ordered behind the conversion
            word_cols[w] = nullptr;
        }
    }
    if (rc != CHGPU_OK)
    {
        chgpu_col_free(k64);
        drop_words();
        return rc;
    }
    if (keys_out)
    {
        if (chgpu_type_size(a->key_type) == 8)
        {
            k64->type = a->key_type;
            *keys_out = k64;
        }
        else
        {
            // insertKeyIntoColumns casts the UInt64 table key back to the column type
            chgpu_col * kn = nullptr;
            rc = chgpu_col_new(ctx, a->key_type, n_out, &kn);
            if (rc == CHGPU_OK && n_out)
            {
                const u32 g2 = chgpu_grid_for(ctx, n_out, 256, 8);
                if (chgpu_type_size(a->key_type) == 4)
                    hipLaunchKernelGGL(k_narrow_keys<u32>, dim3(g2), dim3(256), 0, ctx->stream, (const u64 *)k64->data, n_out, (u32 *)kn->data);
                else if (chgpu_type_size(a->key_type) == 2)
                    hipLaunchKernelGGL(k_narrow_keys<u16>, dim3(g2), dim3(256), 0, ctx->stream, (const u64 *)k64->data, n_out, (u16 *)kn->data);
                else
                    hipLaunchKernelGGL(k_narrow_keys<u8>, dim3(g2), dim3(256), 0, ctx->stream, (const u64 *)k64->data, n_out, (u8 *)kn->data);
                ctx->counters[6] += 1;
            }
            chgpu_col_free(k64); // pooled: any reuse is stream-ordered behind the narrow kernel
            if (rc != CHGPU_OK)
            {
                drop_words();
                return rc;
            }
            *keys_out = kn;
        }
    }
    else
        chgpu_col_free(k64);
    *groups = n_out;
    return CHGPU_OK;
}

extern "C" int chgpu_agg_export_states(chgpu_agg * a, chgpu_col ** keys_out, chgpu_col ** state_cols, uint64_t * groups)
{
    ChgpuDeviceGuard _dev_guard(a ? a->ctx : nullptr);
    CHGPU_REQUIRE(a && state_cols && groups, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    return agg_export(a, keys_out, state_cols, groups);
}

// Two-level form of the partial states: rows ordered by the reference's bucket number, so that block b of a CPU initiator's
// MergingAggregatedMemoryEfficientTransform is a row range.  (The device table itself stays single-level)
extern "C" int chgpu_agg_export_states_two_level(chgpu_agg * a, chgpu_col ** keys_out, chgpu_col ** state_cols, uint64_t * groups, uint64_t * bucket_counts)
{
    ChgpuDeviceGuard _dev_guard(a ? a->ctx : nullptr);
    CHGPU_REQUIRE(a && keys_out && state_cols && groups && bucket_counts, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(a->key_type >= 0, CHGPU_ERR_BAD_ARGUMENTS, "an aggregation without key has no buckets");
    chgpu_col * keys = nullptr;
    chgpu_col * words[AGG_MAX_WORDS] = {nullptr};
    u64 n = 0;
    CHGPU_TRY(agg_export(a, &keys, words, &n));
    const u32 nw = a->words.n_pub_words;
    chgpu_col * sorted[AGG_MAX_WORDS + 1] = {nullptr};
    int rc = CHGPU_OK;
    // <= 8 columns per partition call; the key column rides in the first
    for (u32 lo = 0; lo < nw + 1 && rc == CHGPU_OK; lo += 8)
    {
        const chgpu_col * in[8];
        chgpu_col * out[8] = {nullptr};
        u32 k = 0;
        for (u32 c = lo; c < nw + 1 && k < 8; ++c, ++k)
            in[k] = c == 0 ? keys : words[c - 1];
        rc = chgpu_partition_by_hash(a->ctx, keys, 256, k, in, out, bucket_counts);
        for (u32 j = 0; j < k && rc == CHGPU_OK; ++j)
            sorted[lo + j] = out[j];
    }
    chgpu_col_free(keys);
    for (u32 w = 0; w < nw; ++w)
        chgpu_col_free(words[w]);
    if (rc != CHGPU_OK)
    {
        for (u32 c = 0; c < nw + 1; ++c)
            if (sorted[c])
                chgpu_col_free(sorted[c]);
        return rc;
    }
    *keys_out = sorted[0];
    for (u32 w = 0; w < nw; ++w)
        state_cols[w] = sorted[w + 1];
    *groups = n;
    return CHGPU_OK;
}

// min / max state words (order keys; complemented for min) -> values of the argument's type
__global__ __launch_bounds__(256) void k_extremum_decode(const u64 * __restrict__ words, u64 n, int type, int is_min, void * __restrict__ out)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const u64 bits = is_min == 2 ? words[i] : agg_order_key_inverse(is_min ? ~words[i] : words[i], type);
        switch (type)
        {
            case CHGPU_I64: case CHGPU_U64: case CHGPU_F64: ((u64 *)out)[i] = bits; break;
            case CHGPU_U32: case CHGPU_I32: ((u32 *)out)[i] = (u32)bits; break;
            case CHGPU_U16: case CHGPU_I16: ((u16 *)out)[i] = (u16)bits; break;
            case CHGPU_U8: case CHGPU_I8: ((u8 *)out)[i] = (u8)bits; break;
            case CHGPU_F32: ((float *)out)[i] = (float)__longlong_as_double((long long)bits); break; // the widening was exact: so is this
            default: break;
        }
    }
}

// The results of a conditioned function whose state no row reached: the nested value becomes the type's default where `zero` says so
// (min / max decode an empty word to the type's extremum, a NULL-mode avg divides 0 by 0), and the null map gets its byte.
__global__ __launch_bounds__(256) void k_cond_results(const u64 * __restrict__ reached, u64 n, u32 value_bytes, int zero, void * __restrict__ values,
                                                      u8 * __restrict__ null_map)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const bool empty = reached[i] == 0;
        if (null_map)
            null_map[i] = empty ? 1 : 0;
        if (!empty || !zero)
            continue;
        switch (value_bytes)
        {
            case 8: ((u64 *)values)[i] = 0; break;
            case 4: ((u32 *)values)[i] = 0; break;
            case 2: ((u16 *)values)[i] = 0; break;
            default: ((u8 *)values)[i] = 0; break;
        }
    }
}

static int agg_finalize_impl(chgpu_agg * a, chgpu_col ** keys_out, chgpu_col ** res_cols, chgpu_col ** null_maps, uint64_t * groups)
{
    chgpu_ctx * ctx = a->ctx;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        res_cols[j] = nullptr;
        if (null_maps)
            null_maps[j] = nullptr;
    }
    chgpu_col * words[AGG_MAX_WORDS] = {nullptr};
    u64 n = 0;
    CHGPU_TRY(agg_export(a, keys_out, words, &n));
    int rc = CHGPU_OK;
    for (u32 j = 0; j < a->n_aggs; ++j)
    {
        const u32 w = a->word_off[j];
        if (a->kinds[j] == CHGPU_AGG_COUNT)
        {
            words[w]->type = CHGPU_U64;
            res_cols[j] = words[w];
            words[w] = nullptr;
        }
        else if (a->kinds[j] == CHGPU_AGG_SUM)
        {
            words[w]->type = chgpu_sum_result_type(a->arg_types[j]); // SumSimple: Int64 / UInt64 / Float64
            res_cols[j] = words[w];
            words[w] = nullptr;
        }
        else if (agg_kind(a->kinds[j]).extremum)
        {
            const AggKind & k = agg_kind(a->kinds[j]);
            // insertResultInto: the value itself, in the argument's type (AggregateFunctionsMinMax.cpp)
            chgpu_col * r = nullptr;
            rc = chgpu_col_new(ctx, a->arg_types[j], n, &r);
            if (rc != CHGPU_OK)
                break;
            if (a->key_type < 0 && a->nokey_kept == 0 && a->cond_modes[j] == CHGPU_AGG_COND_NONE) // (a conditioned function: k_cond_results)
                CHGPU_HIP(hipMemsetAsync(r->data, 0, chgpu_type_size(a->arg_types[j]), ctx->stream)); // a state without a value: the type's default
            else if (n)
            {
                // (any, argMin / argMax: the value word, as loaded -- no order key to undo; a cell only a value-less imported state reached holds 0)
                hipLaunchKernelGGL(k_extremum_decode, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream,
                                   (const u64 *)words[w + k.result]->data, n, a->arg_types[j], a->kinds[j] == CHGPU_AGG_MIN ? 1 : k.words > 1 ? 2 : 0, r->data);
                ctx->counters[6] += 1;
            }
            res_cols[j] = r;
        }
        else
        {
            chgpu_col * r = nullptr;
            rc = chgpu_col_new(ctx, CHGPU_F64, n, &r);
            if (rc != CHGPU_OK)
                break;
            if (n)
            {
                hipLaunchKernelGGL(k_avg_divide, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, (const u64 *)words[w]->data,
                                   (const u64 *)words[w + 1]->data, n, chgpu_sum_result_type(a->arg_types[j]), (double *)r->data);
                ctx->counters[6] += 1;
            }
            res_cols[j] = r;
        }
    }
    for (u32 j = 0; j < a->n_aggs && rc == CHGPU_OK; ++j)
    {
        const u32 rw = a->cond_modes[j] == CHGPU_AGG_COND_NONE ? ~0u : agg_reached_word(a, j);
        if (rw == ~0u)
            continue;
        const bool null_mode = a->cond_modes[j] == CHGPU_AGG_COND_NULL;
        if (null_mode && null_maps)
            rc = chgpu_col_new(ctx, CHGPU_U8, n, &null_maps[j]);
        const bool zero = a->kinds[j] == CHGPU_AGG_MIN || a->kinds[j] == CHGPU_AGG_MAX || (null_mode && a->kinds[j] == CHGPU_AGG_AVG);
        if (rc == CHGPU_OK && n && (zero || (null_mode && null_maps)))
        {
            hipLaunchKernelGGL(k_cond_results, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, (const u64 *)words[rw]->data, n,
                               (u32)chgpu_type_size(res_cols[j]->type), zero ? 1 : 0, res_cols[j]->data, (null_mode && null_maps) ? (u8 *)null_maps[j]->data : nullptr);
            ctx->counters[6] += 1;
        }
    }
    for (u32 w = 0; w < a->words.n_pub_words; ++w)
        if (words[w])
            chgpu_col_free(words[w]); // pooled: reuse is stream-ordered behind k_avg_divide / k_cond_results
    if (rc != CHGPU_OK)
        for (u32 j = 0; j < a->n_aggs; ++j)
        {
            if (res_cols[j])
                chgpu_col_free(res_cols[j]), res_cols[j] = nullptr;
            if (null_maps && null_maps[j])
                chgpu_col_free(null_maps[j]), null_maps[j] = nullptr;
        }
    *groups = n;
    return rc;
}

extern "C" int chgpu_agg_finalize(chgpu_agg * a, chgpu_col ** keys_out, chgpu_col ** res_cols, uint64_t * groups)
{
    ChgpuDeviceGuard _dev_guard(a ? a->ctx : nullptr);
    CHGPU_REQUIRE(a && res_cols && groups, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    for (u32 j = 0; j < a->n_aggs; ++j)
        CHGPU_REQUIRE(a->cond_modes[j] != CHGPU_AGG_COND_NULL || a->kinds[j] == CHGPU_AGG_COUNT, CHGPU_ERR_BAD_ARGUMENTS,
                      "function %u has a Nullable result: chgpu_agg_finalize would lose its null map, use chgpu_agg_finalize_nullable", j);
    return agg_finalize_impl(a, keys_out, res_cols, nullptr, groups);
}

extern "C" int chgpu_agg_finalize_nullable(chgpu_agg * a, chgpu_col ** keys_out, chgpu_col ** res_cols, chgpu_col ** null_maps, uint64_t * groups)
{
    ChgpuDeviceGuard _dev_guard(a ? a->ctx : nullptr);
    CHGPU_REQUIRE(a && res_cols && null_maps && groups, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    return agg_finalize_impl(a, keys_out, res_cols, null_maps, groups);
}
