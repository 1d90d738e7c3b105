// pair_store.h — what the operators that keep a flat store of (group key, value) pairs in HBM beside an aggregator share (uniqExact:
// uniq_kernels.hip, quantileExact: quantile_kernels.hip, groupArray: group_array_kernels.hip; the entry helpers also serve
// limit_by_kernels.hip): the element load, the entry checks of create / add_block / merge / the keys look-up, the count() GROUP BY over
// the store's keys, the small launches around them, the append-only store itself (PairStore: reserve, append another store, export) and
// the radix passes over (key, payload) columns.  Pool memory, the numbered allocations and a call's temporaries are pair_pool.h; the
// key -> group table is group_table.h.  A helper here launches and never counts: ctx->counters stay with the caller.  What a helper
// allocates goes through the caller's PairAllocs, in the order its comment states, so every call's numbering is written down
// (test_quantile_fail_alloc).  Kernels are templates or static: several translation units include this file.
#pragma once

#include "chgpu_internal.h"

#include "group_table.h"
#include "pair_host.h"
#include "pair_pool.h"

// raw bits of element i of a column of `size`-byte elements, zero-extended (keys as load_key_zext; values as their own bits)
__device__ __forceinline__ u64 pair_load(const void * p, u32 size, u64 i)
{
    switch (size)
    {
        case 1: return ((const u8 *)p)[i];
        case 2: return ((const u16 *)p)[i];
        case 4: return ((const u32 *)p)[i];
        default: return ((const u64 *)p)[i];
    }
}

static __global__ void k_pair_set_u64(u64 * out, u64 v)
{
    out[0] = v;
}

// UInt64 words back to the column's own width
template <typename T>
__global__ __launch_bounds__(GT_T) void k_pair_narrow(const u64 * __restrict__ in, u64 n, T * __restrict__ out)
{
    for (u64 i = (u64)blockIdx.x * GT_T + threadIdx.x; i < n; i += (u64)gridDim.x * GT_T)
        out[i] = (T)in[i];
}

// what an operator calls itself in its messages, and the head every operator's struct begins with
struct PairNames
{
    const char * op;     // "uniq"
    const char * noun;   // "set"
    const char * a_noun; // "a set"
};

struct PairOp
{
    chgpu_ctx * ctx = nullptr;
    int key_type = -1; // < 0: without key
    int value_type = 0;
};

static chgpu_col pair_view(chgpu_ctx * ctx, int type, void * data, u64 rows)
{
    chgpu_col v;
    v.ctx = ctx;
    v.type = type;
    v.rows = rows;
    v.data = data;
    return v;
}

static int pair_launch_ok(const PairNames & nm, const char * what)
{
    if (hipGetLastError() != hipSuccess)
        return chgpu_set_error(CHGPU_ERR_DEVICE, "%s: %s launch failed", nm.op, what);
    return CHGPU_OK;
}

static void pair_set_u64(chgpu_ctx * ctx, u64 * out, u64 v)
{
    hipLaunchKernelGGL(k_pair_set_u64, dim3(1), dim3(1), 0, ctx->stream, out, v);
}

// n UInt64 words into `out`, an n-row column of a key's or value's type (the words' low bytes); n != 0
static void pair_narrow(chgpu_ctx * ctx, const u64 * words, u64 n, chgpu_col * out)
{
    dispatch_width(chgpu_type_size(out->type), [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(k_pair_narrow<T>, dim3(chgpu_grid_for(ctx, n, GT_T, 8)), dim3(GT_T), 0, ctx->stream, words, n, (T *)out->data);
    });
}

// the `debug` option's line of one call
template <typename Plan>
static void pair_print_plan(chgpu_ctx * ctx, int (*format)(char *, size_t, const Plan &), const Plan & plan)
{
    if (chgpu_opt(ctx, "debug", 0) == 0)
        return;
    char line[512];
    format(line, sizeof(line), plan);
    fprintf(stderr, "%s\n", line);
}

// The groups of a keyed store: count() GROUP BY over its n UInt64 keys, of the rows whose `alive` byte is set (NULL: every row).
// -> the group keys (UInt64), their counts and how many there are; nothing is left allocated when a step fails.
static int pair_count_groups(chgpu_ctx * ctx, void * store_keys, u64 n, const chgpu_col * alive, chgpu_col ** keys, chgpu_col ** counts, u64 * groups)
{
    chgpu_agg * agg = nullptr;
    const int kind = CHGPU_AGG_COUNT, arg_type = CHGPU_U64;
    CHGPU_TRY(chgpu_agg_create(ctx, CHGPU_U64, 1, &kind, &arg_type, 0, &agg));
    const chgpu_col kview = pair_view(ctx, CHGPU_U64, store_keys, n);
    const chgpu_col * args[1] = {nullptr};
    int rc = alive ? chgpu_agg_add_block_filtered(agg, &kview, args, 0, n, alive) : chgpu_agg_add_block(agg, &kview, args, 0, n);
    chgpu_col * res[1] = {nullptr};
    if (rc == CHGPU_OK)
        rc = chgpu_agg_finalize(agg, keys, res, groups);
    *counts = res[0];
    chgpu_agg_free(agg);
    return rc;
}

// ---- entry checks, in the order the calls make them (the caller has checked its own pointers) ----
static int pair_check_create(const PairNames & nm, int key_type, int value_type)
{
    if (key_type >= 0)
    {
        CHGPU_REQUIRE(chgpu_type_size(key_type) != 0, CHGPU_ERR_BAD_ARGUMENTS, "%s: unknown key type %d", nm.op, key_type);
        CHGPU_REQUIRE(chgpu_type_is_int(key_type), CHGPU_ERR_NOT_IMPLEMENTED, "%s: key type %d: integer keys only (CPU path)", nm.op, key_type);
    }
    CHGPU_REQUIRE(chgpu_type_size(value_type) != 0, CHGPU_ERR_BAD_ARGUMENTS, "%s: unknown value type %d", nm.op, value_type);
    return CHGPU_OK;
}

// a, b, c (each may be NULL) live on the operator's device
static int pair_check_device(const PairNames & nm, const PairOp & d, const chgpu_col * a, const chgpu_col * b = nullptr, const chgpu_col * c = nullptr)
{
    const int dev = d.ctx->device;
    CHGPU_REQUIRE((!a || a->ctx->device == dev) && (!b || b->ctx->device == dev) && (!c || c->ctx->device == dev), CHGPU_ERR_BAD_ARGUMENTS,
                  "%s: a column lives on another device than the %s", nm.op, nm.noun);
    return CHGPU_OK;
}

static int pair_check_add_block(const PairNames & nm, const PairOp & d, const chgpu_col * key_col, const chgpu_col * value_col, u64 row_begin, u64 row_end,
                                const chgpu_col * filter_u8)
{
    const bool keyed = d.key_type >= 0;
    CHGPU_REQUIRE(!keyed || key_col, CHGPU_ERR_BAD_ARGUMENTS, "NULL key column");
    CHGPU_REQUIRE(!keyed || key_col->type == d.key_type, CHGPU_ERR_BAD_ARGUMENTS, "%s: key column of type %d, the %s was made for %d", nm.op, key_col->type, nm.noun,
                  d.key_type);
    CHGPU_REQUIRE(value_col->type == d.value_type, CHGPU_ERR_BAD_ARGUMENTS, "%s: value column of type %d, the %s was made for %d", nm.op, value_col->type, nm.noun,
                  d.value_type);
    CHGPU_REQUIRE(!filter_u8 || filter_u8->type == CHGPU_U8, CHGPU_ERR_BAD_ARGUMENTS, "%s: the filter must be UInt8", nm.op);
    CHGPU_TRY(pair_check_device(nm, d, value_col, keyed ? key_col : nullptr, filter_u8));
    const char * msg = "";
    const int code = pair_check_rows(keyed ? (int64_t)key_col->rows : -1, value_col->rows, filter_u8 ? (int64_t)filter_u8->rows : -1, row_begin, row_end, &msg);
    CHGPU_REQUIRE(code == CHGPU_OK, code, "%s: %s", nm.op, msg);
    return CHGPU_OK;
}

static int pair_check_merge(const PairNames & nm, const PairOp & dst, const PairOp & src)
{
    CHGPU_REQUIRE(dst.key_type == src.key_type && dst.value_type == src.value_type, CHGPU_ERR_BAD_ARGUMENTS, "%s: merging %s of (%d, %d) into one of (%d, %d)", nm.op,
                  nm.a_noun, src.key_type, src.value_type, dst.key_type, dst.value_type);
    CHGPU_REQUIRE(dst.ctx->device == src.ctx->device, CHGPU_ERR_BAD_ARGUMENTS, "%s: the %ss live on different devices", nm.op, nm.noun);
    return CHGPU_OK;
}

// the keys column of counts_for_keys / for_keys (its device is checked by pair_check_device, after the caller's own checks)
static int pair_check_keys(const PairNames & nm, const PairOp & d, const chgpu_col * keys)
{
    CHGPU_REQUIRE(d.key_type >= 0, CHGPU_ERR_BAD_ARGUMENTS, "%s: %s without key has no keys to look up", nm.op, nm.a_noun);
    CHGPU_REQUIRE(keys->type == d.key_type, CHGPU_ERR_BAD_ARGUMENTS, "%s: key column of type %d, the %s was made for %d", nm.op, keys->type, nm.noun, d.key_type);
    return CHGPU_OK;
}

// ---- the flat append-only store: u64 keys[cap] (keyed operators) and `width`-byte values[cap], `held` of them in use ----
struct PairStore : PairOp
{
    PairMem k_mem, v_mem;
    u64 held = 0, cap = 0;
    u32 width = 0;
    PairAllocs mem; // the operator's numbered allocations, the store's among them
};

// create, once the arguments are checked: the fields above, and the context is retained
static void pair_store_init(PairStore & s, chgpu_ctx * ctx, int key_type, int value_type, const char * op, const char * fail_option)
{
    s.ctx = ctx;
    s.key_type = key_type < 0 ? -1 : key_type;
    s.value_type = value_type;
    s.width = (u32)chgpu_type_size(value_type);
    s.mem.ctx = ctx;
    s.mem.op = op;
    s.mem.option = fail_option;
    chgpu_ctx_retain(ctx);
}

static void pair_store_free(PairStore & s)
{
    pair_free_mem(s.ctx, s.k_mem);
    pair_free_mem(s.ctx, s.v_mem);
}

// Room for `need` values (the caller has answered its own row limit).  Every allocation first (the keys' when keyed, then the
// values'), so that a failure leaves the store as it was; then what is held is copied.
static int pair_store_reserve(const PairNames & nm, PairStore & s, u64 need)
{
    if (need <= s.cap)
        return CHGPU_OK;
    chgpu_ctx * ctx = s.ctx;
    const bool keyed = s.key_type >= 0;
    const u64 cap = pair_capacity_for(need);
    PairMem k, v;
    int rc = keyed ? s.mem.alloc(cap * 8, &k) : CHGPU_OK;
    if (rc == CHGPU_OK)
        rc = s.mem.alloc(cap * s.width, &v);
    if (rc == CHGPU_OK && s.held)
    {
        hipError_t e = keyed ? hipMemcpyAsync(k.p, s.k_mem.p, s.held * 8, hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
        if (e == hipSuccess)
            e = hipMemcpyAsync(v.p, s.v_mem.p, s.held * s.width, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess)
            rc = chgpu_set_error(CHGPU_ERR_DEVICE, "%s: copying the store failed: %s", nm.op, hipGetErrorString(e));
    }
    if (rc != CHGPU_OK)
    {
        pair_free_mem(ctx, k);
        pair_free_mem(ctx, v);
        return rc;
    }
    pair_store_free(s); // reuse is ordered behind the copies above (same stream)
    s.k_mem = k;
    s.v_mem = v;
    s.cap = cap;
    return CHGPU_OK;
}

// merge: the whole of `src` behind what `dst` holds; dst may be src.  reserve(need) is the operator's own reserve, with its row limit.
// after_copies() runs on dst's stream behind the two copies and BEFORE the wait that lets the source change: what else the operator
// reads of the source (groupArray's key words) is launched there.
template <typename Reserve, typename After>
static int pair_store_append_store(const PairNames & nm, PairStore & dst, const PairStore & src, Reserve reserve, After after_copies)
{
    chgpu_ctx * ctx = dst.ctx;
    const u64 n = src.held;
    if (n == 0)
        return CHGPU_OK;
    if (src.ctx != ctx && hipStreamSynchronize(src.ctx->stream) != hipSuccess) // src's values were written on its own stream
        return chgpu_set_error(CHGPU_ERR_DEVICE, "%s: waiting for the source failed", nm.op);
    CHGPU_TRY(reserve(dst.held + n));
    const bool keyed = dst.key_type >= 0;
    hipError_t e = keyed ? hipMemcpyAsync((u64 *)dst.k_mem.p + dst.held, src.k_mem.p, n * 8, hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
    if (e == hipSuccess)
        e = hipMemcpyAsync((char *)dst.v_mem.p + dst.held * dst.width, src.v_mem.p, n * dst.width, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess)
        after_copies();
    if (e == hipSuccess && src.ctx != ctx)
        e = hipStreamSynchronize(ctx->stream); // src may change once this returns
    if (e != hipSuccess)
        return chgpu_set_error(CHGPU_ERR_DEVICE, "%s: copying the source's store failed: %s", nm.op, hipGetErrorString(e));
    dst.held += n;
    return CHGPU_OK;
}

// export_pairs behind the caller's NULL checks: the keys column (keyed operators) and the values column are allocated in that order,
// the keys narrowed to their type; export_values(column) launches or enqueues the operator's own copy of the values and counts both.
template <typename Values>
static int pair_store_export(const PairNames & nm, PairStore & s, chgpu_col ** keys_out, chgpu_col ** values_out, uint64_t * rows, Values export_values)
{
    const bool keyed = s.key_type >= 0;
    CHGPU_REQUIRE(!keyed || keys_out, CHGPU_ERR_BAD_ARGUMENTS, "NULL keys_out");
    ChgpuDeviceGuard guard(s.ctx);
    s.mem.begin_call();
    chgpu_col * k = nullptr;
    chgpu_col * v = nullptr;
    int rc = keyed ? s.mem.col_new(s.key_type, s.held, &k) : CHGPU_OK;
    if (rc == CHGPU_OK)
        rc = s.mem.col_new(s.value_type, s.held, &v);
    if (rc == CHGPU_OK && s.held)
    {
        if (keyed)
            pair_narrow(s.ctx, (const u64 *)s.k_mem.p, s.held, k);
        rc = export_values(v);
        if (rc == CHGPU_OK)
            rc = pair_launch_ok(nm, "export");
    }
    if (rc != CHGPU_OK)
    {
        if (k) chgpu_col_free(k);
        if (v) chgpu_col_free(v);
        return rc;
    }
    if (keys_out)
        *keys_out = k;
    *values_out = v;
    *rows = s.held;
    return CHGPU_OK;
}

// ---- radix passes over (key column, payload column) ----
// Pass p is one stable 256-way chgpu_partition_by_key_byte by the key's byte at shifts[p] and counts as ONE allocation of the call (its
// two output columns).  cur[2]: the input on entry (it stays the caller's), the last pass's output on return.  own[2]: NULL on entry;
// the columns of the latest pass, the caller's to free (its temporaries): a pass's input is freed as soon as the next pass has replaced
// it (reuse is ordered on the stream behind the pass that read it), so at most two generations are alive.
static int pair_run_passes(PairAllocs & mem, const u32 * shifts, u32 passes, const chgpu_col * cur[2], chgpu_col ** own /* [2] */)
{
    for (u32 p = 0; p < passes; ++p)
    {
        CHGPU_TRY(mem.refused());
        chgpu_col * outs[2] = {nullptr, nullptr};
        CHGPU_TRY(chgpu_partition_by_key_byte(mem.ctx, cur[0], shifts[p], 2, cur, outs));
        for (u32 c = 0; c < 2; ++c)
        {
            if (own[c]) chgpu_col_free(own[c]);
            own[c] = outs[c];
            cur[c] = outs[c];
        }
    }
    return CHGPU_OK;
}
