// pair_store.h — what the operators that keep a flat store of (group key, value) pairs in HBM beside an aggregator share (uniqExact:
// uniq_kernels.hip, quantileExact: quantile_kernels.hip): the element load, the pool memory they own, the entry checks of create /
// add_block / merge / the keys look-up, the count() GROUP BY over the store's keys, and the small launches around them.  The key ->
// group table is group_table.h.  A helper here launches and never counts or allocates: ctx->counters and every allocation stay with
// the caller, which numbers them (test_quantile_fail_alloc).  Kernels are templates or static: two translation units include this file.
#pragma once

#include "chgpu_internal.h"

#include "group_table.h"
#include "pair_host.h"

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

// memory from the context's pool
struct PairMem
{
    void * p = nullptr;
    size_t cls = 0;
};

static void pair_free_mem(chgpu_ctx * ctx, PairMem & m)
{
    if (m.p)
        chgpu_pool_free(ctx, m.p, m.cls);
    m = PairMem{};
}

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
