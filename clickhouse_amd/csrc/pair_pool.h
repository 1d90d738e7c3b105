// pair_pool.h — the pool memory an operator owns, the numbered allocations of one call and the call's temporaries, written once for
// quantile_kernels.hip, group_array_kernels.hip, limit_by_kernels.hip, window_kernels.hip, merge_kernels.hip, merge_fold_kernels.hip
// and the ColumnString operators (string_column.h).  Host code only, and nothing of group_table.h or pair_store.h comes with it.
#pragma once

#include <vector>

#include "chgpu_internal.h"

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

// The allocations of one call, numbered from 1 in the order they are asked for.  Test hook: with `option` set to N, allocation N of a
// call answers OOM, which is how the tests reach every error path behind an allocation.  option == NULL: no hook (window).
struct PairAllocs
{
    chgpu_ctx * ctx = nullptr;
    const char * op = nullptr;     // "quantile"
    const char * option = nullptr; // "test_quantile_fail_alloc"
    long long fail = 0, seq = 0;

    void begin_call()
    {
        seq = 0;
        fail = option ? chgpu_opt(ctx, option, 0) : 0;
    }
    // counts one allocation of the call (a step that allocates inside another routine is counted by calling this in front of it)
    int refused()
    {
        seq += 1;
        if (fail && seq == fail)
            return chgpu_set_error(CHGPU_ERR_OOM, "%s: allocation %lld refused (%s)", op, seq, option);
        return CHGPU_OK;
    }
    int alloc(size_t bytes, PairMem * m)
    {
        CHGPU_TRY(refused());
        return chgpu_pool_alloc(ctx, bytes ? bytes : 256, &m->p, &m->cls);
    }
    int col_new(int type, u64 rows, chgpu_col ** out)
    {
        CHGPU_TRY(refused());
        return chgpu_col_new(ctx, type, rows, out);
    }
};

// temporaries of one call, freed when it ends (reuse of the memory is ordered on the stream behind the kernels that read it)
struct PairTemps
{
    PairAllocs & mem;
    std::vector<PairMem> mems;
    std::vector<chgpu_col *> cols; // (an entry may be NULL)
    explicit PairTemps(PairAllocs & a) : mem(a) {}
    ~PairTemps()
    {
        for (PairMem & m : mems)
            pair_free_mem(mem.ctx, m);
        for (chgpu_col * c : cols)
            if (c) chgpu_col_free(c);
    }
    int alloc(size_t bytes, void ** out)
    {
        PairMem m;
        CHGPU_TRY(mem.alloc(bytes, &m));
        mems.push_back(m);
        *out = m.p;
        return CHGPU_OK;
    }
    // gives one allocation back before the call ends (a round of the string sort); its emptied entry stays
    void release(void * p)
    {
        for (PairMem & m : mems)
            if (m.p == p) pair_free_mem(mem.ctx, m);
    }
    int col(int type, u64 rows, chgpu_col ** out)
    {
        CHGPU_TRY(mem.col_new(type, rows, out));
        cols.push_back(*out);
        return CHGPU_OK;
    }
};
