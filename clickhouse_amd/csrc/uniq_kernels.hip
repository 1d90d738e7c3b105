// uniq_kernels.hip — uniqExact / count(DISTINCT x) under GROUP BY: one flat, exact set of (group key, value) pairs in HBM.
//
// Reference (file:line in the reference checkout):
//   AggregateFunctionUniqExact: a HashSet<T> per group      src/AggregateFunctions/AggregateFunctionUniq.h (AggregateFunctionUniqExactData)
//   the cell compares with bitEquals                          src/Common/HashTable/HashTable.h (HashTableCell::keyEquals)
//   count(DISTINCT x) = uniqExact(x)                          count_distinct_implementation, src/Core/Settings.cpp
//
// Design (not a translation).  A per-group set needs per-group allocation; one set of pairs does not, merges by union and finalises as
// a count() GROUP BY over the distinct pairs' keys, which chgpu_agg already does.
//   store  u64 keys[limit], u64 values[limit]: pair k, written once by the lane that took slot k (append-only; one atomic per wave)
//   table  u64 cells[capacity]: {32-bit fingerprint of the pair's hash << 32 | store index + 1}; 0 = empty
// Insert walk (uq_walk): a lane probes read-only until it finds its pair (done) or an empty cell; there it takes a store slot, writes
// the pair, release-fences and only then compare-and-swaps the cell from empty -- so every non-empty cell a reader meets points at a
// complete pair, nobody waits for another lane inside a kernel, and no verify pass or sentinel value is needed.  A failed swap walks on
// from that cell with the same slot.  If two workgroups insert one new pair at once the loser meets the winner's cell further on: its
// slot stays a HOLE.  A slot is alive exactly when looking its pair up returns its own index; size = slots - holes.  A fingerprint
// mismatch skips the store read, a match is always confirmed on the bytes: the set is exact.
// Pairs cross workgroups inside one launch, and an L1 is never refreshed by another CU's stores: cells and store are read and written
// with agent-scope accesses in the insert kernels (they bypass the L1); kernels that run later read them plainly.
//   LDS stage (k_uq_insert_tiles): a workgroup puts a tile of UQ_TILE rows into LDS and inserts them into an LDS set whose cell holds
//   the claiming ROW's index in the tile (one 32-bit compare-and-swap; the pair itself is immutable, so no cell is ever half written).
//   Only the rows that claimed a cell -- the tile's distinct pairs -- and the rows that found no room go on to the global table.
//   Growth: the table holds capacity / 2 pairs.  A row that would insert beyond that sets its bit in the chunk's pending bitmap; the host
//   grows the table (x4 to 2^23 cells, then x2), rebuilds the cells from the store and runs the pending rows again (k_uq_insert_pending).
// What this operator shares with quantile_kernels.hip (element load, pool memory, entry checks, the groups of the store's keys, the
// key -> group table) is pair_store.h / group_table.h.
#include "chgpu_internal.h"

#include "pair_store.h"
#include "uniq_host.h"

typedef unsigned long long ull;

static constexpr u32 UQ_T = 256;                   // threads of every kernel here
static constexpr u32 UQ_R = 8;                     // rows per lane of a tile
static constexpr u32 UQ_TILE = UQ_T * UQ_R;        // 2048 rows: 32 KiB of pairs in LDS
static constexpr u32 UQ_LDS_LG_CELLS = 10;
static constexpr u32 UQ_LDS_CELLS = 1u << UQ_LDS_LG_CELLS; // cells of the workgroup's LDS set: half a tile, so a tile of distinct pairs overflows it
static constexpr u32 UQ_LDS_PROBES = 16;           // cells a row looks at in the LDS set before it goes to the global table directly
static constexpr u64 UQ_KEY_MULT = 0x9E3779B97F4A7C15ull; // odd: key -> key * UQ_KEY_MULT is a bijection
static constexpr u32 UQ_NO_SLOT = 0xFFFFFFFFu;
static constexpr u64 UQ_CHUNK_ROWS = 64ull << 20;  // rows per pass (bounds the pending bitmap and the rows one growth re-runs)
static constexpr u64 UQ_FIRST_CHUNK_ROWS = 4ull << 20;
static constexpr u32 UQ_FLAG_DEFERRED = 1, UQ_FLAG_FATAL = 2, UQ_FLAG_TODO = 4; // TODO: k_uq_lookup left rows for k_uq_insert_tiles
static constexpr u32 UQ_LOOKUP_U = 4;              // rows per lane of k_uq_lookup, all their loads in flight together

struct UqCtrl
{
    u32 n_slots; // store slots handed out (may pass the limit: slots at or beyond it are never written)
    u32 holes;
    u32 flags;
    u32 pad;
    ull lds, sent, ovf, deferred, found; // the plan line's counts for one launch
};

struct UqTable
{
    u64 * cells;
    u64 capacity; // power of two
    u64 * store_k;
    u64 * store_v;
    u64 limit;        // slots of the store = pairs the table takes: capacity / 2
    u32 slots_before; // slots handed out before this launch
    UqCtrl * ctrl;
};

struct UqSrc
{
    const void * key;
    u32 key_size; // bytes per key element; 0: without key, every row has key 0
    const void * val;
    u32 val_size;
    const u8 * filter; // may be NULL
};

// Placement hash of a pair.  For a fixed key a bijection of the value, for a fixed value a bijection of the key (an odd multiply, an
// xor and intHash64 are each one): tests/uniq_craft.py inverts it to make pairs with a chosen home cell.
//   global home cell = hash & (capacity - 1)    fingerprint = hash >> 32    LDS home cell = hash >> (64 - UQ_LDS_LG_CELLS)
__device__ __forceinline__ u64 uq_hash(u64 key, u64 val)
{
    return dev_intHash64(val ^ key * UQ_KEY_MULT);
}

__device__ __forceinline__ u64 uq_ld(const u64 * p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void uq_st(u64 * p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// what a thread gathers over a kernel; flushed once per wave
struct UqTally
{
    u32 known; // what this wave knows of the slot counter: the host's count at launch, then whatever its own claims returned
    u32 holes = 0, flags = 0;
    u32 lds = 0, sent = 0, ovf = 0, deferred = 0, found = 0;
};

// The insert walk, wave-synchronous: every iteration each active lane looks at one cell; the lanes that need a slot in this iteration
// take them with one atomic for the whole wave.  Call with the wave converged.  my: the lane's store slot (k_uq_rebuild brings one),
// else UQ_NO_SLOT.  -> true: the row met the limit and must run again after the table has grown.
__device__ __forceinline__ bool uq_walk(const UqTable & t, bool active, u64 key, u64 val, u32 my, UqTally & y)
{
    const u64 mask = t.capacity - 1;
    const u64 h = uq_hash(key, val);
    const u32 fp = (u32)(h >> 32);
    u64 pos = h & mask;
    bool deferred = false;
    // (a lane spends at most one extra iteration per cell, the one in which it takes its slot)
    for (u64 step = 0; __any(active); ++step)
    {
        if (step > 2 * t.capacity + 4)
        {
            y.flags |= UQ_FLAG_FATAL; // cannot happen while the cells are at most half full
            break;
        }
        bool want = false;
        if (active)
        {
            u64 c = uq_ld(t.cells + pos);
            if (c == 0)
            {
                if (my == UQ_NO_SLOT)
                {
                    if (y.known >= t.limit)
                    {
                        deferred = true; // the table grows first
                        active = false;
                    }
                    else
                        want = true;
                }
                else
                {
                    c = atomicCAS((ull *)(t.cells + pos), 0ull, ((ull)fp << 32) | ((ull)my + 1));
                    if (c == 0)
                        active = false; // inserted
                }
            }
            if (active && !want)
            {
                // a cell that is not empty: its pair is complete (written and released before the cell was)
                bool same = false;
                if ((u32)(c >> 32) == fp)
                {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); // the store reads stay behind the cell's
                    const u64 idx = (u64)(u32)c - 1;
                    same = uq_ld(t.store_k + idx) == key && uq_ld(t.store_v + idx) == val;
                }
                if (same)
                {
                    y.holes += my != UQ_NO_SLOT; // the pair went in under another slot meanwhile: mine is a hole
                    active = false;
                }
                else
                    pos = (pos + 1) & mask;
            }
        }
        const u64 wanters = __ballot(want);
        if (wanters)
        {
            u32 base = 0;
            const u32 leader = (u32)__ffsll((long long)wanters) - 1;
            if (lane_id() == leader)
                base = atomicAdd(&t.ctrl->n_slots, (u32)__popcll(wanters));
            base = __shfl(base, (int)leader, 64);
            y.known = base + (u32)__popcll(wanters);
            if (want)
            {
                const u32 s = base + mbcnt(wanters);
                if (s < t.limit) // never write past the store
                {
                    my = s;
                    uq_st(t.store_k + s, key);
                    uq_st(t.store_v + s, val);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); // the pair is out before the cell that points at it
                }
                else
                {
                    deferred = true;
                    active = false;
                }
            }
        }
    }
    if (active)
        y.flags |= UQ_FLAG_FATAL;
    if (deferred)
    {
        y.flags |= UQ_FLAG_DEFERRED;
        y.deferred += 1;
    }
    return deferred;
}

__device__ __forceinline__ void uq_flush_tally(const UqTable & t, const UqTally & y, bool count_holes)
{
    u32 flags = y.flags;
    for (int o = 32; o > 0; o >>= 1)
        flags |= __shfl_xor(flags, o, 64);
    const u32 holes = wave_reduce_add_u32(y.holes), lds = wave_reduce_add_u32(y.lds), sent = wave_reduce_add_u32(y.sent), ovf = wave_reduce_add_u32(y.ovf),
              deferred = wave_reduce_add_u32(y.deferred), found = wave_reduce_add_u32(y.found);
    if (lane_id() != 0)
        return;
    if (found) atomicAdd(&t.ctrl->found, (ull)found);
    if (flags) atomicOr(&t.ctrl->flags, flags);
    if (holes && count_holes) atomicAdd(&t.ctrl->holes, holes);
    if (lds) atomicAdd(&t.ctrl->lds, (ull)lds);
    if (sent) atomicAdd(&t.ctrl->sent, (ull)sent);
    if (ovf) atomicAdd(&t.ctrl->ovf, (ull)ovf);
    if (deferred) atomicAdd(&t.ctrl->deferred, (ull)deferred);
}

// before every launch that inserts: the device's control block is the host's view, flags and counts cleared -- whatever exit the
// call before this one took
__global__ void k_uq_ctrl_reset(UqCtrl * c, u32 n_slots, u32 holes)
{
    c->n_slots = n_slots;
    c->holes = holes;
    c->flags = 0;
    c->pad = 0;
    c->lds = c->sent = c->ovf = c->deferred = c->found = 0;
}

// The set as it stood before this chunk, looked up with no loop and no atomics: UQ_LOOKUP_U rows per lane, every load unconditional, so a
// lane has its rows' cell loads, then their store loads in flight together (the walk has one).  A row is settled when its HOME cell
// holds its pair under a slot of an earlier launch -- such a cell and its pair are visible to plain loads; every other row (a new pair,
// a displaced one, one inserted by this very call's launches only in part) gets its bit in `todo` and goes through k_uq_insert_tiles.
__global__ __launch_bounds__(UQ_T) void k_uq_lookup(UqTable t, UqSrc s, u64 row_begin, u64 n, ull * __restrict__ todo)
{
    const u64 mask = t.capacity - 1;
    const u64 stride = (u64)gridDim.x * UQ_T;
    UqTally y;
    y.known = 0;
    u32 any_todo = 0;
    for (u64 i0 = (u64)blockIdx.x * UQ_T + threadIdx.x; i0 < n; i0 += stride * UQ_LOOKUP_U)
    {
        u64 key[UQ_LOOKUP_U], val[UQ_LOOKUP_U], c[UQ_LOOKUP_U], sk[UQ_LOOKUP_U], sv[UQ_LOOKUP_U];
        u32 fp[UQ_LOOKUP_U];
        bool in[UQ_LOOKUP_U];
#pragma unroll
        for (u32 u = 0; u < UQ_LOOKUP_U; ++u)
        {
            const u64 i = i0 + u * stride;
            const u64 r = row_begin + (i < n ? i : n - 1);
            in[u] = i < n && (!s.filter || s.filter[r] != 0);
            key[u] = s.key_size ? pair_load(s.key, s.key_size, r) : 0;
            val[u] = pair_load(s.val, s.val_size, r);
        }
#pragma unroll
        for (u32 u = 0; u < UQ_LOOKUP_U; ++u)
        {
            const u64 h = uq_hash(key[u], val[u]);
            fp[u] = (u32)(h >> 32);
            c[u] = t.cells[h & mask];
        }
#pragma unroll
        for (u32 u = 0; u < UQ_LOOKUP_U; ++u)
        {
            const u64 idx = (u64)(u32)c[u] - 1; // 2^32 - 1 for an empty cell
            const bool cand = c[u] != 0 && (u32)(c[u] >> 32) == fp[u] && idx < t.slots_before;
            c[u] = cand;
            sk[u] = t.store_k[cand ? idx : 0];
            sv[u] = t.store_v[cand ? idx : 0];
        }
#pragma unroll
        for (u32 u = 0; u < UQ_LOOKUP_U; ++u)
        {
            const u64 i = i0 + u * stride;
            const bool settled = c[u] && sk[u] == key[u] && sv[u] == val[u];
            const bool need = in[u] && !settled;
            y.found += in[u] && settled;
            const ull w = __ballot(need); // the wave's rows are 64 consecutive ones from a multiple of 64
            if (w != 0 && lane_id() == (u32)__ffsll((long long)__ballot(true)) - 1)
                todo[i >> 6] = w;
            any_todo |= w != 0;
        }
    }
    if (any_todo)
        y.flags |= UQ_FLAG_TODO;
    uq_flush_tally(t, y, false);
}

// Rows [row_begin, row_begin + n) by tiles through the LDS set.  pending: one bit per row of the chunk, zeroed by the host.  todo: NULL, or
// the rows k_uq_lookup left (the launch before this one; it raised UQ_FLAG_TODO if there are any).
__global__ __launch_bounds__(UQ_T) void k_uq_insert_tiles(UqTable t, UqSrc s, u64 row_begin, u64 n, ull * __restrict__ pending, const ull * __restrict__ todo)
{
    if (todo && !(t.ctrl->flags & UQ_FLAG_TODO)) // the look-up settled every row
        return;
    __shared__ u64 lk[UQ_TILE];
    __shared__ u64 lv[UQ_TILE];
    __shared__ u32 lcell[UQ_LDS_CELLS]; // claiming row's index in the tile + 1; 0 = empty
    __shared__ u32 list[UQ_TILE];       // the rows sent on
    __shared__ u32 n_list;
    const u32 tid = threadIdx.x;
    UqTally y;
    y.known = t.slots_before;
    const u64 tiles = (n + UQ_TILE - 1) / UQ_TILE;
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    {
        for (u32 c = tid; c < UQ_LDS_CELLS; c += UQ_T)
            lcell[c] = 0;
        if (tid == 0)
            n_list = 0;
        u64 kk[UQ_R], vv[UQ_R];
        u32 act = 0;
#pragma unroll
        for (u32 r = 0; r < UQ_R; ++r)
        {
            const u32 j = r * UQ_T + tid;
            const u64 i = tile * UQ_TILE + j;
            bool a = i < n;
            if (a && todo)
                a = (todo[i >> 6] >> (i & 63)) & 1; // (the filter is in the bit already)
            else if (a && s.filter)
                a = s.filter[row_begin + i] != 0;
            kk[r] = a && s.key_size ? pair_load(s.key, s.key_size, row_begin + i) : 0;
            vv[r] = a ? pair_load(s.val, s.val_size, row_begin + i) : 0;
            lk[j] = kk[r];
            lv[j] = vv[r];
            act |= (u32)a << r;
        }
        __syncthreads(); // every pair of the tile is in LDS, the set is empty
#pragma unroll
        for (u32 r = 0; r < UQ_R; ++r)
        {
            const u32 j = r * UQ_T + tid;
            bool send = false;
            if ((act >> r) & 1)
            {
                u32 pos = (u32)(uq_hash(kk[r], vv[r]) >> (64 - UQ_LDS_LG_CELLS));
                bool done = false;
#pragma unroll 1
                for (u32 p = 0; p < UQ_LDS_PROBES && !done; ++p)
                {
                    u32 c = ((volatile u32 *)lcell)[pos];
                    if (c == 0)
                    {
                        c = atomicCAS(&lcell[pos], 0u, j + 1);
                        if (c == 0)
                        {
                            send = done = true; // this row stands for its pair
                            break;
                        }
                    }
                    // the claimer's pair was in LDS before the barrier and never changes
                    if (lk[c - 1] == kk[r] && lv[c - 1] == vv[r])
                    {
                        done = true;
                        y.lds += 1;
                    }
                    else
                        pos = (pos + 1) & (UQ_LDS_CELLS - 1);
                }
                if (!done)
                {
                    send = true; // no room around its home cell: straight to the global table
                    y.ovf += 1;
                }
            }
            y.sent += send;
            const u64 senders = __ballot(send);
            if (senders)
            {
                u32 base = 0;
                const u32 leader = (u32)__ffsll((long long)senders) - 1;
                if (lane_id() == leader)
                    base = atomicAdd(&n_list, (u32)__popcll(senders));
                base = __shfl(base, (int)leader, 64);
                if (send)
                    list[base + mbcnt(senders)] = j;
            }
        }
        __syncthreads(); // the list is complete
        const u32 m = n_list;
        for (u32 e0 = 0; e0 < m; e0 += UQ_T)
        {
            const u32 e = e0 + tid;
            const bool active = e < m;
            const u32 j = active ? list[e] : 0;
            if (uq_walk(t, active, lk[j], lv[j], UQ_NO_SLOT, y))
            {
                const u64 i = tile * UQ_TILE + j;
                atomicOr(&pending[i >> 6], 1ull << (i & 63));
            }
        }
        __syncthreads(); // before the next tile overwrites LDS
    }
    uq_flush_tally(t, y, true);
}

// The rows whose pending bit is set, straight into the global table (after a growth); a row that defers again keeps its bit.
__global__ __launch_bounds__(UQ_T) void k_uq_insert_pending(UqTable t, UqSrc s, u64 row_begin, u64 n, ull * __restrict__ pending)
{
    UqTally y;
    y.known = t.slots_before;
    const u32 lane = lane_id();
    const u64 words = (n + 63) / 64, waves = (u64)gridDim.x * (UQ_T / 64);
    for (u64 g = ((u64)blockIdx.x * UQ_T + threadIdx.x) / 64; g < words; g += waves)
    {
        const ull w = pending[g]; // one word per wave
        if (w == 0)
            continue;
        const bool active = (w >> lane) & 1;
        const u64 i = row_begin + g * 64 + lane;
        const u64 key = active && s.key_size ? pair_load(s.key, s.key_size, i) : 0;
        const u64 val = active ? pair_load(s.val, s.val_size, i) : 0;
        const bool deferred = uq_walk(t, active, key, val, UQ_NO_SLOT, y);
        const ull again = __ballot(deferred);
        if (lane == 0)
            pending[g] = again;
    }
    uq_flush_tally(t, y, true);
}

// growth / roll-back: the cells from the store.  Slot k goes in under its own index; a hole meets its pair's other slot and stays one.
__global__ __launch_bounds__(UQ_T) void k_uq_rebuild(UqTable t, u64 n_slots)
{
    UqTally y;
    y.known = 0;
    for (u64 b = (u64)blockIdx.x * UQ_T; b < n_slots; b += (u64)gridDim.x * UQ_T)
    {
        const u64 k = b + threadIdx.x;
        const bool active = k < n_slots;
        const u64 key = active ? t.store_k[k] : 0, val = active ? t.store_v[k] : 0;
        uq_walk(t, active, key, val, active ? (u32)k : 0u, y);
    }
    uq_flush_tally(t, y, false); // the holes are the ones the host already counts
}

// read-only look-up in a table no kernel is writing: the pair's store index, or UQ_NO_SLOT
__device__ __forceinline__ u32 uq_find(const UqTable & t, u64 key, u64 val)
{
    const u64 mask = t.capacity - 1;
    const u64 h = uq_hash(key, val);
    const u32 fp = (u32)(h >> 32);
    u64 pos = h & mask;
    for (u64 step = 0; step <= t.capacity; ++step)
    {
        const u64 c = t.cells[pos];
        if (c == 0)
            break;
        if ((u32)(c >> 32) == fp)
        {
            const u64 idx = (u64)(u32)c - 1;
            if (t.store_k[idx] == key && t.store_v[idx] == val)
                return (u32)idx;
        }
        pos = (pos + 1) & mask;
    }
    return UQ_NO_SLOT;
}

// alive[k] = 1 when slot k is the one its pair is found under
__global__ __launch_bounds__(UQ_T) void k_uq_alive(UqTable t, u64 n_slots, u8 * __restrict__ alive)
{
    for (u64 k = (u64)blockIdx.x * UQ_T + threadIdx.x; k < n_slots; k += (u64)gridDim.x * UQ_T)
        alive[k] = uq_find(t, t.store_k[k], t.store_v[k]) == (u32)k;
}

// counts_for_keys: the table over the finalised groups (group_table.h)
__global__ __launch_bounds__(UQ_T) void k_uq_kc_lookup(const u64 * __restrict__ gkeys, const u64 * __restrict__ gcounts, const u32 * __restrict__ cells, u64 cap,
                                                       const void * __restrict__ keys, u32 key_size, u64 n, u64 * __restrict__ out)
{
    for (u64 i = (u64)blockIdx.x * UQ_T + threadIdx.x; i < n; i += (u64)gridDim.x * UQ_T)
    {
        const u32 g = gt_find(gkeys, cells, cap, pair_load(keys, key_size, i));
        out[i] = g == GT_NONE ? 0 : gcounts[g];
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static constexpr PairNames UQ_NAMES{"uniq", "set", "a set"};

struct chgpu_uniq : PairOp
{
    UqTable t{};
    PairMem cells_mem, sk_mem, sv_mem, ctrl_mem;
    u64 n_slots = 0, holes = 0;
    // what finalize computed, kept until the set changes: the groups (UInt64 keys, counts); the key -> group table of counts_for_keys
    bool fin_valid = false;
    chgpu_col * fin_keys = nullptr;
    chgpu_col * fin_counts = nullptr;
    u64 fin_groups = 0;
    PairMem kc_mem;
    u64 kc_cap = 0;
    long long fail_growth = 0; // test hook: the growth with this number (1 = first of a call) answers OOM, so that the roll-back runs
};

static void uq_drop_final(chgpu_uniq * d)
{
    if (d->fin_keys) chgpu_col_free(d->fin_keys);
    if (d->fin_counts) chgpu_col_free(d->fin_counts);
    d->fin_keys = d->fin_counts = nullptr;
    d->fin_groups = 0;
    pair_free_mem(d->ctx, d->kc_mem);
    d->kc_cap = 0;
    d->fin_valid = false;
}

static int uq_rebuild(chgpu_uniq * d, u64 n_slots)
{
    chgpu_ctx * ctx = d->ctx;
    CHGPU_HIP(hipMemsetAsync(d->t.cells, 0, d->t.capacity * 8, ctx->stream));
    if (!n_slots)
        return CHGPU_OK;
    hipLaunchKernelGGL(k_uq_ctrl_reset, dim3(1), dim3(1), 0, ctx->stream, d->t.ctrl, (u32)n_slots, (u32)d->holes);
    hipLaunchKernelGGL(k_uq_rebuild, dim3(chgpu_grid_for(ctx, n_slots, UQ_T, 8)), dim3(UQ_T), 0, ctx->stream, d->t, n_slots);
    ctx->counters[6] += 2;
    ctx->counters[7] += 1;
    return pair_launch_ok(UQ_NAMES, "rebuild");
}

// A table of `cap` cells (and a store of its limit) in place of the present one: every allocation first, so that a failure leaves the
// object exactly as it was; then the store is copied and the cells rebuilt from it.
static int uq_resize(chgpu_uniq * d, u64 cap)
{
    chgpu_ctx * ctx = d->ctx;
    const u64 limit = uq_limit(cap);
    PairMem cells, sk, sv;
    int rc = chgpu_pool_alloc(ctx, cap * 8, &cells.p, &cells.cls);
    if (rc == CHGPU_OK) rc = chgpu_pool_alloc(ctx, limit * 8, &sk.p, &sk.cls);
    if (rc == CHGPU_OK) rc = chgpu_pool_alloc(ctx, limit * 8, &sv.p, &sv.cls);
    if (rc != CHGPU_OK)
    {
        pair_free_mem(ctx, cells);
        pair_free_mem(ctx, sk);
        pair_free_mem(ctx, sv);
        return rc;
    }
    if (d->n_slots)
    {
        hipError_t e = hipMemcpyAsync(sk.p, d->t.store_k, d->n_slots * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(sv.p, d->t.store_v, d->n_slots * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess)
        {
            pair_free_mem(ctx, cells);
            pair_free_mem(ctx, sk);
            pair_free_mem(ctx, sv);
            return chgpu_set_error(CHGPU_ERR_DEVICE, "uniq: copying the store failed: %s", hipGetErrorString(e));
        }
    }
    pair_free_mem(ctx, d->cells_mem); // reuse is ordered behind the copies above (same stream)
    pair_free_mem(ctx, d->sk_mem);
    pair_free_mem(ctx, d->sv_mem);
    d->cells_mem = cells;
    d->sk_mem = sk;
    d->sv_mem = sv;
    d->t.cells = (u64 *)cells.p;
    d->t.store_k = (u64 *)sk.p;
    d->t.store_v = (u64 *)sv.p;
    d->t.capacity = cap;
    d->t.limit = limit;
    return uq_rebuild(d, d->n_slots);
}

// Rows [row_begin, row_begin + n) of `s` into the set.  On an error the set holds exactly what it held at entry.
static int uq_add_rows(chgpu_uniq * d, const UqSrc & s, u64 row_begin, u64 n, const char * what)
{
    chgpu_ctx * ctx = d->ctx;
    UqPlan plan;
    plan.what = what;
    plan.n = n;
    plan.cap_before = d->t.capacity;
    plan.slots_before = d->n_slots;
    plan.holes_before = d->holes;
    const u64 entry_slots = d->n_slots, entry_holes = d->holes;
    int rc = CHGPU_OK;
    if (n)
        uq_drop_final(d);
    u64 chunk = UQ_FIRST_CHUNK_ROWS;
    for (u64 c0 = 0, m = 0; c0 < n && rc == CHGPU_OK; c0 += m, chunk = chunk * 4 < UQ_CHUNK_ROWS ? chunk * 4 : UQ_CHUNK_ROWS)
    {
        m = n - c0 < chunk + chunk / 2 ? n - c0 : chunk; // a short tail joins the last chunk
        const u64 tiles = (m + UQ_TILE - 1) / UQ_TILE;
        const u64 max_grid = (u64)ctx->num_cus * 3; // three workgroups' LDS fit a CU
        const u32 grid = (u32)(tiles < max_grid ? tiles : max_grid);
        void * scratch = nullptr;
        const size_t pending_bytes = ((size_t)((m + 63) / 64) * 8 + 255) / 256 * 256;
        if ((rc = chgpu_scratch(ctx, 2 * pending_bytes, &scratch)) != CHGPU_OK)
            break;
        ull * pending = (ull *)scratch;
        ull * todo = (ull *)((char *)scratch + pending_bytes);
        // a set that holds something: most rows of a later block find their pair in its home cell, and the loop-free look-up settles those
        const bool lookup_first = d->n_slots != 0;
        if (hipMemsetAsync(pending, 0, (lookup_first ? 2 : 1) * pending_bytes, ctx->stream) != hipSuccess)
        {
            rc = chgpu_set_error(CHGPU_ERR_DEVICE, "uniq: clearing the pending rows failed");
            break;
        }
        plan.chunks += 1;
        plan.tiles += tiles;
        for (u32 round = 0; rc == CHGPU_OK; ++round)
        {
            d->t.slots_before = (u32)d->n_slots;
            hipLaunchKernelGGL(k_uq_ctrl_reset, dim3(1), dim3(1), 0, ctx->stream, d->t.ctrl, (u32)d->n_slots, (u32)d->holes);
            if (round == 0 && lookup_first)
            {
                hipLaunchKernelGGL(k_uq_lookup, dim3(chgpu_grid_for(ctx, (m + UQ_LOOKUP_U - 1) / UQ_LOOKUP_U, UQ_T, 8)), dim3(UQ_T), 0, ctx->stream, d->t, s, row_begin + c0, m, todo);
                ctx->counters[6] += 1;
            }
            if (round == 0)
                hipLaunchKernelGGL(k_uq_insert_tiles, dim3(grid), dim3(UQ_T), 0, ctx->stream, d->t, s, row_begin + c0, m, pending, lookup_first ? (const ull *)todo : nullptr);
            else
                hipLaunchKernelGGL(k_uq_insert_pending, dim3(chgpu_grid_for(ctx, m, UQ_T, 4)), dim3(UQ_T), 0, ctx->stream, d->t, s, row_begin + c0, m, pending);
            ctx->counters[6] += 2;
            if ((rc = pair_launch_ok(UQ_NAMES, "insert")) != CHGPU_OK)
                break;
            UqCtrl c; // the one blocking read of a round: 56 bytes
            if ((rc = chgpu_read_back(ctx, d->t.ctrl, &c, sizeof(c))) != CHGPU_OK)
                break;
            d->n_slots = c.n_slots < d->t.limit ? c.n_slots : d->t.limit; // slots past the limit were handed out but never written
            d->holes = c.holes;
            plan.lds += c.lds;
            plan.sent += c.sent;
            plan.ovf += c.ovf;
            plan.deferred += c.deferred;
            plan.found += c.found;
            if (c.flags & UQ_FLAG_FATAL)
            {
                rc = chgpu_set_error(CHGPU_ERR_LOGICAL, "uniq: a walk did not end in a table at most half full");
                break;
            }
            if (!(c.flags & UQ_FLAG_DEFERRED))
                break;
            // rows wait at the limit: the next capacity, the cells rebuilt from the store, the pending rows again
            if (d->t.capacity >= UQ_CAP_MAX)
            {
                rc = chgpu_set_error(CHGPU_ERR_TOO_MANY_ROWS, "uniq: more than %llu distinct pairs", (unsigned long long)UQ_MAX_SLOTS);
                break;
            }
            plan.grown += 1;
            if (d->fail_growth && (long long)plan.grown == d->fail_growth)
                rc = chgpu_set_error(CHGPU_ERR_OOM, "uniq: growth %u refused (test_uniq_fail_growth)", plan.grown);
            else
                rc = uq_resize(d, uq_grow(d->t.capacity));
        }
    }
    if (rc != CHGPU_OK && n)
    {
        // roll back: the slots of this call are dropped and the cells rebuilt from the ones before it (a hole's pair and the slot it
        // lost to were both inserted by one earlier call or by calls before it: the holes at entry are the holes among those slots)
        d->n_slots = entry_slots;
        d->holes = entry_holes;
        const int saved_rc = rc;
        std::string saved_msg = chgpu_last_error();
        if (uq_rebuild(d, entry_slots) == CHGPU_OK)
            (void)hipStreamSynchronize(ctx->stream);
        rc = chgpu_set_error(saved_rc, "%s", saved_msg.c_str());
    }
    plan.cap = d->t.capacity;
    plan.slots = d->n_slots;
    plan.holes = d->holes;
    plan.rc = rc;
    pair_print_plan(ctx, uq_format_plan, plan);
    return rc;
}

// alive mask of `d`'s slots as a UInt8 column of `ctx` (the kernel runs on ctx's stream)
static int uq_alive(const chgpu_uniq * d, chgpu_ctx * ctx, chgpu_col ** out)
{
    chgpu_col * alive = nullptr;
    CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U8, d->n_slots, &alive));
    if (d->n_slots)
    {
        hipLaunchKernelGGL(k_uq_alive, dim3(chgpu_grid_for(ctx, d->n_slots, UQ_T, 8)), dim3(UQ_T), 0, ctx->stream, d->t, d->n_slots, (u8 *)alive->data);
        ctx->counters[6] += 1;
        const int rc = pair_launch_ok(UQ_NAMES, "alive");
        if (rc != CHGPU_OK)
        {
            chgpu_col_free(alive);
            return rc;
        }
    }
    *out = alive;
    return CHGPU_OK;
}

// a UInt64 column as a column of `type` (the words' low bytes)
static int uq_narrow(chgpu_ctx * ctx, const u64 * words, u64 n, int type, chgpu_col ** out)
{
    chgpu_col * c = nullptr;
    CHGPU_TRY(chgpu_col_new(ctx, type, n, &c));
    if (n)
    {
        pair_narrow(ctx, words, n, c);
        ctx->counters[6] += 1;
        const int rc = pair_launch_ok(UQ_NAMES, "narrow");
        if (rc != CHGPU_OK)
        {
            chgpu_col_free(c);
            return rc;
        }
    }
    *out = c;
    return CHGPU_OK;
}

// the groups of a keyed set: count() GROUP BY over the alive slots' keys
static int uq_finalize_groups(chgpu_uniq * d)
{
    if (d->fin_valid)
        return CHGPU_OK;
    chgpu_ctx * ctx = d->ctx;
    uq_drop_final(d);
    chgpu_col * keys = nullptr;
    chgpu_col * counts = nullptr;
    u64 groups = 0;
    if (d->n_slots == 0)
    {
        CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, 0, &keys));
        const int rc = chgpu_col_new(ctx, CHGPU_U64, 0, &counts);
        if (rc != CHGPU_OK)
        {
            chgpu_col_free(keys);
            return rc;
        }
    }
    else
    {
        chgpu_col * alive = nullptr;
        CHGPU_TRY(uq_alive(d, ctx, &alive));
        const int rc = pair_count_groups(ctx, d->t.store_k, d->n_slots, alive, &keys, &counts, &groups);
        chgpu_col_free(alive);
        if (rc != CHGPU_OK)
            return rc;
    }
    d->fin_keys = keys;
    d->fin_counts = counts;
    d->fin_groups = groups;
    d->fin_valid = true;
    return CHGPU_OK;
}

// the key -> group table of counts_for_keys, built on its first call after the groups were
static int uq_key_table(chgpu_uniq * d)
{
    CHGPU_TRY(uq_finalize_groups(d));
    if (d->kc_mem.p)
        return CHGPU_OK;
    chgpu_ctx * ctx = d->ctx;
    const u64 groups = d->fin_groups;
    CHGPU_REQUIRE(groups < 0xFFFFFFFFull, CHGPU_ERR_TOO_MANY_ROWS, "uniq: more than 2^32 - 2 groups");
    const u64 cap = gt_capacity_for(groups);
    PairMem kc;
    CHGPU_TRY(chgpu_pool_alloc(ctx, cap * 4, &kc.p, &kc.cls));
    int rc = gt_fill(ctx, UQ_NAMES.op, (const u64 *)d->fin_keys->data, groups, (u32 *)kc.p, cap);
    if (rc == CHGPU_OK && groups)
    {
        ctx->counters[6] += 1;
        rc = pair_launch_ok(UQ_NAMES, "key table");
    }
    if (rc != CHGPU_OK)
    {
        pair_free_mem(ctx, kc);
        return rc;
    }
    d->kc_mem = kc;
    d->kc_cap = cap;
    return CHGPU_OK;
}

extern "C" int chgpu_uniq_create(chgpu_ctx * ctx, int key_type, int value_type, uint64_t size_hint, chgpu_uniq ** out)
{
    CHGPU_REQUIRE(ctx && out, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_create(UQ_NAMES, key_type, value_type));
    const u64 cap = uq_capacity_for(size_hint);
    CHGPU_REQUIRE(cap != 0, CHGPU_ERR_TOO_MANY_ROWS, "uniq: a size hint of %llu pairs, at most %llu fit", (unsigned long long)size_hint, (unsigned long long)UQ_MAX_SLOTS);
    ChgpuDeviceGuard guard(ctx);
    chgpu_uniq * d = new chgpu_uniq();
    d->ctx = ctx;
    d->key_type = key_type < 0 ? -1 : key_type;
    d->value_type = value_type;
    d->fail_growth = chgpu_opt(ctx, "test_uniq_fail_growth", 0);
    chgpu_ctx_retain(ctx);
    int rc = chgpu_pool_alloc(ctx, 256, &d->ctrl_mem.p, &d->ctrl_mem.cls);
    if (rc == CHGPU_OK)
    {
        d->t.ctrl = (UqCtrl *)d->ctrl_mem.p;
        rc = uq_resize(d, cap);
    }
    if (rc != CHGPU_OK)
    {
        chgpu_uniq_free(d);
        return rc;
    }
    *out = d;
    return CHGPU_OK;
}

extern "C" int chgpu_uniq_free(chgpu_uniq * d)
{
    if (!d)
        return CHGPU_OK;
    ChgpuDeviceGuard guard(d->ctx);
    uq_drop_final(d);
    pair_free_mem(d->ctx, d->cells_mem);
    pair_free_mem(d->ctx, d->sk_mem);
    pair_free_mem(d->ctx, d->sv_mem);
    pair_free_mem(d->ctx, d->ctrl_mem);
    chgpu_ctx * ctx = d->ctx;
    delete d;
    chgpu_ctx_release(ctx);
    return CHGPU_OK;
}

extern "C" int chgpu_uniq_add_block(chgpu_uniq * d, const chgpu_col * key_col, const chgpu_col * value_col, uint64_t row_begin, uint64_t row_end,
                                    const chgpu_col * filter_u8)
{
    CHGPU_REQUIRE(d && value_col, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_add_block(UQ_NAMES, *d, key_col, value_col, row_begin, row_end, filter_u8));
    const bool keyed = d->key_type >= 0;
    ChgpuDeviceGuard guard(d->ctx);
    UqSrc s{};
    s.key = keyed ? key_col->data : nullptr;
    s.key_size = keyed ? (u32)chgpu_type_size(d->key_type) : 0;
    s.val = value_col->data;
    s.val_size = (u32)chgpu_type_size(d->value_type);
    s.filter = filter_u8 ? (const u8 *)filter_u8->data : nullptr;
    return uq_add_rows(d, s, row_begin, row_end - row_begin, "add");
}

extern "C" int chgpu_uniq_merge(chgpu_uniq * dst, const chgpu_uniq * src)
{
    CHGPU_REQUIRE(dst && src, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_merge(UQ_NAMES, *dst, *src));
    if (dst == src)
        return CHGPU_OK;
    chgpu_ctx * ctx = dst->ctx;
    ChgpuDeviceGuard guard(ctx);
    if (src->ctx != ctx) // src's pairs were written on its own stream
        CHGPU_HIP(hipStreamSynchronize(src->ctx->stream));
    chgpu_col * alive = nullptr;
    CHGPU_TRY(uq_alive(src, ctx, &alive));
    UqSrc s{};
    s.key = src->t.store_k;
    s.key_size = dst->key_type >= 0 ? 8 : 0;
    s.val = src->t.store_v;
    s.val_size = 8;
    s.filter = (const u8 *)alive->data;
    int rc = uq_add_rows(dst, s, 0, src->n_slots, "merge");
    if (rc == CHGPU_OK && src->ctx != ctx && hipStreamSynchronize(ctx->stream) != hipSuccess) // src may change once this returns
        rc = chgpu_set_error(CHGPU_ERR_DEVICE, "uniq: waiting for the merge failed");
    chgpu_col_free(alive);
    return rc;
}

extern "C" int chgpu_uniq_size(chgpu_uniq * d, uint64_t * pairs)
{
    CHGPU_REQUIRE(d && pairs, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    *pairs = d->n_slots - d->holes;
    return CHGPU_OK;
}

extern "C" int chgpu_uniq_export_pairs(chgpu_uniq * d, chgpu_col ** keys_out, chgpu_col ** values_out, uint64_t * pairs)
{
    CHGPU_REQUIRE(d && values_out && pairs, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    const bool keyed = d->key_type >= 0;
    CHGPU_REQUIRE(!keyed || keys_out, CHGPU_ERR_BAD_ARGUMENTS, "NULL keys_out");
    chgpu_ctx * ctx = d->ctx;
    ChgpuDeviceGuard guard(ctx);
    chgpu_col * k64 = nullptr;
    chgpu_col * v64 = nullptr;
    chgpu_col * kout = nullptr;
    chgpu_col * vout = nullptr;
    u64 rows = 0;
    int rc = CHGPU_OK;
    if (d->n_slots)
    {
        chgpu_col * alive = nullptr;
        CHGPU_TRY(uq_alive(d, ctx, &alive));
        const chgpu_col kview = pair_view(ctx, CHGPU_U64, d->t.store_k, d->n_slots), vview = pair_view(ctx, CHGPU_U64, d->t.store_v, d->n_slots);
        if (keyed)
            rc = chgpu_filter(ctx, &kview, alive, 0, &k64, &rows);
        if (rc == CHGPU_OK)
            rc = chgpu_filter(ctx, &vview, alive, 0, &v64, &rows);
        chgpu_col_free(alive);
    }
    if (rc == CHGPU_OK && keyed)
        rc = uq_narrow(ctx, k64 ? (const u64 *)k64->data : nullptr, rows, d->key_type, &kout);
    if (rc == CHGPU_OK)
        rc = uq_narrow(ctx, v64 ? (const u64 *)v64->data : nullptr, rows, d->value_type, &vout);
    if (k64) chgpu_col_free(k64);
    if (v64) chgpu_col_free(v64);
    if (rc != CHGPU_OK)
    {
        if (kout) chgpu_col_free(kout);
        return rc;
    }
    if (keys_out)
        *keys_out = kout;
    *values_out = vout;
    *pairs = rows;
    return CHGPU_OK;
}

extern "C" int chgpu_uniq_finalize(chgpu_uniq * d, chgpu_col ** keys_out, chgpu_col ** counts_u64, uint64_t * groups)
{
    CHGPU_REQUIRE(d && counts_u64 && groups, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    const bool keyed = d->key_type >= 0;
    CHGPU_REQUIRE(!keyed || keys_out, CHGPU_ERR_BAD_ARGUMENTS, "NULL keys_out");
    chgpu_ctx * ctx = d->ctx;
    ChgpuDeviceGuard guard(ctx);
    if (!keyed)
    {
        // without key: exactly one row, 0 for the empty set
        chgpu_col * c = nullptr;
        CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, 1, &c));
        pair_set_u64(ctx, (u64 *)c->data, d->n_slots - d->holes);
        ctx->counters[6] += 1;
        const int rc = pair_launch_ok(UQ_NAMES, "finalize");
        if (rc != CHGPU_OK)
        {
            chgpu_col_free(c);
            return rc;
        }
        if (keys_out)
            *keys_out = nullptr;
        *counts_u64 = c;
        *groups = 1;
        return CHGPU_OK;
    }
    CHGPU_TRY(uq_finalize_groups(d));
    chgpu_col * k = nullptr;
    chgpu_col * c = nullptr;
    CHGPU_TRY(uq_narrow(ctx, (const u64 *)d->fin_keys->data, d->fin_groups, d->key_type, &k));
    int rc = chgpu_col_new(ctx, CHGPU_U64, d->fin_groups, &c);
    if (rc == CHGPU_OK && d->fin_groups && hipMemcpyAsync(c->data, d->fin_counts->data, d->fin_groups * 8, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
        rc = chgpu_set_error(CHGPU_ERR_DEVICE, "uniq: copying the counts failed");
    if (rc != CHGPU_OK)
    {
        chgpu_col_free(k);
        if (c) chgpu_col_free(c);
        return rc;
    }
    *keys_out = k;
    *counts_u64 = c;
    *groups = d->fin_groups;
    return CHGPU_OK;
}

extern "C" int chgpu_uniq_counts_for_keys(chgpu_uniq * d, const chgpu_col * keys, chgpu_col ** counts_u64)
{
    CHGPU_REQUIRE(d && keys && counts_u64, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_keys(UQ_NAMES, *d, keys));
    CHGPU_TRY(pair_check_device(UQ_NAMES, *d, keys));
    chgpu_ctx * ctx = d->ctx;
    ChgpuDeviceGuard guard(ctx);
    CHGPU_TRY(uq_key_table(d));
    chgpu_col * c = nullptr;
    CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, keys->rows, &c));
    if (keys->rows)
    {
        hipLaunchKernelGGL(k_uq_kc_lookup, dim3(chgpu_grid_for(ctx, keys->rows, UQ_T, 8)), dim3(UQ_T), 0, ctx->stream, (const u64 *)d->fin_keys->data,
                           (const u64 *)d->fin_counts->data, (const u32 *)d->kc_mem.p, d->kc_cap, keys->data, (u32)chgpu_type_size(d->key_type), keys->rows, (u64 *)c->data);
        ctx->counters[6] += 1;
        const int rc = pair_launch_ok(UQ_NAMES, "counts_for_keys");
        if (rc != CHGPU_OK)
        {
            chgpu_col_free(c);
            return rc;
        }
    }
    *counts_u64 = c;
    return CHGPU_OK;
}
