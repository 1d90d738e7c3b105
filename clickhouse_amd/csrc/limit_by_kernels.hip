// limit_by_kernels.hip — SELECT DISTINCT and LIMIT n [OFFSET m] BY key as one streaming operator: a growing key -> counter table in HBM
// and, per block, a UInt8 filter that says which rows pass.
//
// Reference: DistinctTransform::transform / buildFilter and LimitByTransform::transform (src/Processors/Transforms): a hash map from the
// SipHash128 of the key columns to a counter, walked row by row; `if (count++ >= offset && count <= offset + length) pass`.
//
// Design (not a translation).  A row passes by its OCCURRENCE NUMBER k = counter at entry + rank among the block's rows
// of the same key, in row order.
//   table     u64 cells[cap] (open addressing, linear probing from intHash64(key) & (cap - 1), at most half full): a cell IS the key,
//             claimed whole with one 64-bit compare-and-swap from 0; key 0 lives out of line in slot `cap`.  u32 count[cap + 1] and
//             u32 claim[cap + 1] run parallel to the cells; a row's slot is its cell index.  A cell never changes once set, so a stale
//             read can only show "empty" and the failed swap corrects it; a lane never waits for another lane.
//   resolve   k_lb_resolve: four consecutive rows per lane, every load of a stage unconditional (keys in one 4 / 8 / 16 / 32-byte
//             access, home cells, counters).  A row is dead when its filter byte is 0 or its counter has reached offset + length; the
//             rest are live; a live row whose key the table lacks is marked missing.  Per tile the live count, per call the totals and
//             the OR / AND words of the live slots.  Missing rows: k_lb_insert (find or insert, keys handed out against the limit by
//             wave-aggregated tickets), the table grows while a round meets the limit, then the block is resolved AGAIN by the same
//             find-only kernel: no slot taken before a growth is used after it and no rank is taken before every row has its slot.
//   records   k_lb_compact: the live rows as (slot, row), in row order, by tile counts -> scan -> ballot ranks.
//   claim     offset + length == 1: k_lb_claim_min leaves min(row) in claim[slot] (equal slots reduced in LDS first: at most one global
//             atomic per workgroup, tile and slot), k_lb_claim_pass passes the row that holds its slot's claim, sets the counter and puts
//             the claim back to "none".
//   rank      one stable 256-way pass of chgpu_partition_by_key_byte over (slot, row) per slot byte that varies among the live records;
//             equal slots are then adjacent and in row order.  Segment heads by counts -> scan -> ballot ranks, rank = position - head,
//             filter[row] = offset <= count + rank < offset + length; the counters are raised in a launch of their own (one lane per
//             segment), so no lane reads a counter another lane of the launch writes.
// Counters and claims are written only after the call's last allocation: a call that answers OOM leaves every counter as it was.
// Shared with group_array_kernels.hip and written once elsewhere: the rank plan's head ballots, counts kernel, ranked-item loop and
// tile scan (tile_rank.h), its pass planner and pass loop (pair_host.h, pair_store.h); the numbered allocations and the call's
// temporaries are pair_pool.h.  k_lb_compact and k_lb_resolve rank lane-consecutive rows, another layout, and stay as they are.
#include "block_scan.h"

#include "pair_store.h"
#include "tile_rank.h"
#include "limit_by_host.h"

static constexpr u32 LB_T = TILE_T;         // threads of every kernel here
static constexpr u32 LB_V = 4;              // consecutive rows of a lane in the resolve and compaction kernels
static constexpr u32 LB_R = TILE_R;         // steps of LB_T records a workgroup takes of a record tile in the claim plan
static constexpr u32 LB_RTILE = TILE_ITEMS; // records of a record tile: the claim plan's, and tile_rank.h's tile in the rank plan
static constexpr u32 LB_LDS_CELLS = 1024; // the claim plan's workgroup set
static constexpr u32 LB_LDS_PROBES = 16;

static_assert(LB_TILE == (u64)LB_T * LB_V, "a tile is four rows of every thread");

// rewritten (zeroed) from the host's view before every launch sequence that reads it: no flag of an earlier call is ever seen
struct LbCtl
{
    u32 entered, live, missing; // resolve
    u32 or_bits, nand_bits;     // resolve: OR of the live slots, OR of their complements
    u32 tickets, inserted, overflow; // insert
    u32 passed, counted;        // apply: rows that pass, slots whose counter left 0
    u32 pad[6];
};

template <typename K>
struct alignas(sizeof(K) * LB_V) LbVec
{
    K v[LB_V];
};

struct alignas(16) LbSlots
{
    u32 v[LB_V];
};

// Rows are addressed by v = row - row_begin + lead, where `lead` (< 4) makes v = 0 fall on a 4-element boundary of the key column's
// memory; kp / fp point at the range's first row.  slot_out[v]: the live row's slot, LB_MISSING, or LB_NONE.
template <typename K>
__global__ __launch_bounds__(LB_T) void k_lb_resolve(const K * __restrict__ kp, const u8 * __restrict__ fp, u32 lead, u64 vn, u64 n_tiles, const u64 * __restrict__ cells,
                                                     u64 cap, const u32 * __restrict__ count, u32 bound, u32 * __restrict__ slot_out, u32 * __restrict__ tile_counts,
                                                     LbCtl * ctl)
{
    __shared__ u32 s_tile, s_acc[5];
    const u64 mask = cap - 1;
    u32 entered = 0, live = 0, missing = 0, ob = 0, nb = 0;
    if (threadIdx.x == 0)
        s_tile = 0;
    if (threadIdx.x < 5)
        s_acc[threadIdx.x] = 0;
    __syncthreads();
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    {
        const u64 v0 = tile * LB_TILE + (u64)threadIdx.x * LB_V;
        const i64 i0 = (i64)v0 - (i64)lead;
        const bool whole = v0 >= lead && v0 + LB_V <= vn; // all four rows are rows of the range: one wide access
        u64 k[LB_V];
        bool in[LB_V];
        // stage 1: keys and filter bytes
        if (whole)
        {
            const LbVec<K> kv = *(const LbVec<K> *)(kp + i0);
#pragma unroll
            for (u32 j = 0; j < LB_V; ++j)
            {
                k[j] = kv.v[j];
                in[j] = true;
            }
            if (fp)
            {
                if ((((uintptr_t)(fp + i0)) & 3) == 0)
                {
                    const u32 w = *(const u32 *)(fp + i0);
#pragma unroll
                    for (u32 j = 0; j < LB_V; ++j)
                        in[j] = ((w >> (8 * j)) & 0xFF) != 0;
                }
                else
                {
#pragma unroll
                    for (u32 j = 0; j < LB_V; ++j)
                        in[j] = fp[i0 + j] != 0;
                }
            }
        }
        else
        {
#pragma unroll
            for (u32 j = 0; j < LB_V; ++j)
            {
                const bool valid = v0 + j >= lead && v0 + j < vn;
                k[j] = valid ? (u64)kp[i0 + j] : 0;
                in[j] = valid && (!fp || fp[i0 + j] != 0);
            }
        }
        // stage 2: home cells
        u64 pos[LB_V], c[LB_V];
#pragma unroll
        for (u32 j = 0; j < LB_V; ++j)
        {
            pos[j] = dev_intHash64(k[j]) & mask;
            c[j] = cells[pos[j]];
        }
        // stage 3: the walk of a row that is not at home (the table is at most half full: an empty cell ends it)
        u32 slot[LB_V];
#pragma unroll
        for (u32 j = 0; j < LB_V; ++j)
        {
            if (k[j] == 0)
                slot[j] = (u32)cap; // the empty value's own slot: always there
            else
            {
                u64 p = pos[j], cc = c[j];
                if (in[j])
                    for (u64 step = 0; cc != k[j] && cc != 0 && step < cap; ++step)
                    {
                        p = (p + 1) & mask;
                        cc = cells[p];
                    }
                slot[j] = cc == k[j] ? (u32)p : LB_MISSING;
            }
        }
        // stage 4: counters
        u32 cnt[LB_V];
#pragma unroll
        for (u32 j = 0; j < LB_V; ++j)
            cnt[j] = count[slot[j] == LB_MISSING ? 0u : slot[j]];
        LbSlots out;
        u32 tile_live = 0;
#pragma unroll
        for (u32 j = 0; j < LB_V; ++j)
        {
            const bool miss = in[j] && slot[j] == LB_MISSING;
            const bool lv = in[j] && (miss || cnt[j] < bound);
            out.v[j] = lv ? slot[j] : LB_NONE;
            entered += in[j];
            tile_live += lv;
            missing += miss;
            if (lv && !miss)
            {
                ob |= slot[j];
                nb |= ~slot[j];
            }
        }
        *(LbSlots *)(slot_out + v0) = out; // (slot_out holds n_tiles whole tiles)
        live += tile_live;
        tile_live = wave_reduce_add_u32(tile_live);
        if (lane_id() == 0)
            atomicAdd(&s_tile, tile_live);
        __syncthreads();
        if (threadIdx.x == 0)
        {
            tile_counts[tile] = s_tile;
            s_tile = 0;
        }
        __syncthreads();
    }
    entered = wave_reduce_add_u32(entered);
    live = wave_reduce_add_u32(live);
    missing = wave_reduce_add_u32(missing);
    ob = wave_reduce_all<OrU32>(ob);
    nb = wave_reduce_all<OrU32>(nb);
    if (lane_id() == 0)
    {
        atomicAdd(&s_acc[0], entered);
        atomicAdd(&s_acc[1], live);
        atomicAdd(&s_acc[2], missing);
        atomicOr(&s_acc[3], ob);
        atomicOr(&s_acc[4], nb);
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        atomicAdd(&ctl->entered, s_acc[0]);
        atomicAdd(&ctl->live, s_acc[1]);
        atomicAdd(&ctl->missing, s_acc[2]);
        atomicOr(&ctl->or_bits, s_acc[3]);
        atomicOr(&ctl->nand_bits, s_acc[4]);
    }
}

// The rows resolve marked missing find or insert their key.  A lane that meets an empty cell takes a ticket first (one atomic per
// wave for the lanes that are there together); tickets at or beyond `room` insert nothing and raise `overflow`: cells taken <= tickets
// honoured <= room, so the table never passes its limit whatever the lanes' timing.  A ticket whose swap loses to the same key is
// spent: the limit is met early, never late.  Once `overflow` is seen a lane takes no further row.
template <typename K>
__global__ __launch_bounds__(LB_T) void k_lb_insert(const K * __restrict__ kp, u32 lead, u64 vn, const u32 * __restrict__ slot_in, u64 * cells, u64 cap, u32 room, LbCtl * ctl)
{
    const u64 mask = cap - 1;
    for (u64 v = (u64)blockIdx.x * LB_T + threadIdx.x; v < vn; v += (u64)gridDim.x * LB_T)
    {
        // the limit is met: the host grows the table and runs the missing rows again.  One read per wave and step (the first active
        // lane's, handed to the others): 1e8 reads of this one address cost a block of new keys 90 ms
        u32 met = 0;
        if (mbcnt(__ballot(1)) == 0)
            met = __hip_atomic_load(&ctl->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__builtin_amdgcn_readfirstlane(met))
            return;
        if (v < lead || slot_in[v] != LB_MISSING)
            continue;
        const u64 k = (u64)kp[(i64)v - (i64)lead];
        u64 pos = dev_intHash64(k) & mask;
        bool ticket = false;
        for (u64 step = 0; step <= cap; ++step)
        {
            const u64 c = __hip_atomic_load(&cells[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c == k)
                break;
            if (c == 0)
            {
                if (!ticket)
                {
                    const u64 together = __ballot(1);
                    const u32 leader = (u32)__ffsll((long long)together) - 1;
                    u32 first = 0;
                    if (lane_id() == leader)
                        first = atomicAdd(&ctl->tickets, (u32)__popcll(together));
                    first = __shfl(first, leader, WAVE);
                    if (first + mbcnt(together) >= room)
                    {
                        atomicOr(&ctl->overflow, 1u);
                        break;
                    }
                    ticket = true;
                }
                const u64 old = atomicCAS((unsigned long long *)&cells[pos], 0ull, (unsigned long long)k);
                if (old == 0)
                {
                    atomicAdd(&ctl->inserted, 1u);
                    break;
                }
                if (old == k)
                    break;
            }
            pos = (pos + 1) & mask;
        }
    }
}

// growth: every key of the old table into the new one (cleared by the host), its counter with it; the empty value's slot too
__global__ __launch_bounds__(LB_T) void k_lb_rehash(const u64 * __restrict__ old_cells, const u32 * __restrict__ old_count, u64 old_cap, u64 * cells, u32 * __restrict__ count,
                                                    u64 cap)
{
    const u64 mask = cap - 1;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        count[cap] = old_count[old_cap];
    for (u64 i = (u64)blockIdx.x * LB_T + threadIdx.x; i < old_cap; i += (u64)gridDim.x * LB_T)
    {
        const u64 k = old_cells[i];
        if (k == 0)
            continue;
        u64 pos = dev_intHash64(k) & mask;
        for (u64 step = 0; step <= cap; ++step)
        {
            if (__hip_atomic_load(&cells[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 &&
                atomicCAS((unsigned long long *)&cells[pos], 0ull, (unsigned long long)k) == 0)
            {
                count[pos] = old_count[i];
                break;
            }
            pos = (pos + 1) & mask;
        }
    }
}

// the live rows of tile t as records at tile_off[t] + their rank in the tile; the order (wave, lane, row of the lane) is row order
__global__ __launch_bounds__(LB_T) void k_lb_compact(const u32 * __restrict__ slot_in, u32 lead, u64 n_tiles, const u64 * __restrict__ tile_off, u64 n_live,
                                                     u32 * __restrict__ rec_slot, u32 * __restrict__ rec_row)
{
    __shared__ u32 s_wave[LB_T / 64];
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    {
        const u64 v0 = tile * LB_TILE + (u64)threadIdx.x * LB_V;
        const LbSlots s = *(const LbSlots *)(slot_in + v0);
        u32 below = 0, mine = 0, total = 0;
#pragma unroll
        for (u32 j = 0; j < LB_V; ++j)
        {
            const u64 m = __ballot(s.v[j] != LB_NONE);
            below += mbcnt(m);
            total += (u32)__popcll(m);
        }
        if (lane_id() == 0)
            s_wave[threadIdx.x >> 6] = total;
        __syncthreads();
        u64 at = tile_off[tile] + below;
        for (u32 w = 0; w < (threadIdx.x >> 6); ++w)
            at += s_wave[w];
#pragma unroll
        for (u32 j = 0; j < LB_V; ++j)
        {
            if (s.v[j] != LB_NONE)
            {
                if (at + mine < n_live) // (the counts were taken from these slots)
                {
                    rec_slot[at + mine] = s.v[j];
                    rec_row[at + mine] = (u32)(v0 + j - lead);
                }
                mine += 1;
            }
        }
        __syncthreads(); // before the next tile overwrites the counts
    }
}

// ---- plan claim ---------------------------------------------------------------------------------------------------------------
// claim[slot] = min(row) over the live records.  A tile's records go through a workgroup set in LDS (slot -> lowest row, one 32-bit
// compare-and-swap per cell); what the set holds after the tile is at most one global atomic per slot, skipped when the claim read
// is already lower.  A record that finds no room within LB_LDS_PROBES cells goes to the global claim itself.
__global__ __launch_bounds__(LB_T) void k_lb_claim_min(const u32 * __restrict__ rec_slot, const u32 * __restrict__ rec_row, u64 n_live, u64 n_tiles, u32 * claim)
{
    __shared__ u32 s_slot[LB_LDS_CELLS], s_row[LB_LDS_CELLS];
    for (u32 c = threadIdx.x; c < LB_LDS_CELLS; c += LB_T)
    {
        s_slot[c] = LB_NONE;
        s_row[c] = LB_NONE;
    }
    __syncthreads();
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    {
#pragma unroll 2
        for (u32 r = 0; r < LB_R; ++r)
        {
            const u64 i = tile * LB_RTILE + (u64)r * LB_T + threadIdx.x;
            if (i >= n_live)
                continue;
            const u32 slot = rec_slot[i], row = rec_row[i];
            u32 h = (slot * 0x9E3779B1u) >> 22;
            bool placed = false;
            for (u32 p = 0; p < LB_LDS_PROBES && !placed; ++p)
            {
                const u32 old = atomicCAS(&s_slot[h], LB_NONE, slot);
                if (old == LB_NONE || old == slot)
                {
                    atomicMin(&s_row[h], row);
                    placed = true;
                }
                h = (h + 1) & (LB_LDS_CELLS - 1);
            }
            if (!placed && __hip_atomic_load(&claim[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > row)
                atomicMin(&claim[slot], row);
        }
        __syncthreads();
        for (u32 c = threadIdx.x; c < LB_LDS_CELLS; c += LB_T)
        {
            const u32 slot = s_slot[c];
            if (slot != LB_NONE)
            {
                const u32 row = s_row[c];
                if (__hip_atomic_load(&claim[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > row)
                    atomicMin(&claim[slot], row);
                s_slot[c] = LB_NONE;
                s_row[c] = LB_NONE;
            }
        }
        __syncthreads();
    }
}

// a workgroup's count into the control block: every thread calls it
__device__ __forceinline__ void lb_fold_count(u32 v, u32 * dst)
{
    v = wave_reduce_add_u32(v);
    if (lane_id() == 0 && v)
        atomicAdd(dst, v);
}

// exactly the record that holds its slot's claim passes: it sets the counter and puts the claim back (every other record of the slot
// reads that row or "none", never its own)
__global__ __launch_bounds__(LB_T) void k_lb_claim_pass(const u32 * __restrict__ rec_slot, const u32 * __restrict__ rec_row, u64 n_live, u32 * claim, u32 * __restrict__ count,
                                                        u8 * __restrict__ filter, u64 n, LbCtl * ctl)
{
    u32 passed = 0;
    for (u64 i = (u64)blockIdx.x * LB_T + threadIdx.x; i < n_live; i += (u64)gridDim.x * LB_T)
    {
        const u32 slot = rec_slot[i], row = rec_row[i];
        if (claim[slot] == row && row < n)
        {
            filter[row] = 1;
            count[slot] = 1;
            claim[slot] = LB_NONE;
            passed += 1;
        }
    }
    lb_fold_count(passed, &ctl->passed);
}

// ---- plan rank ----------------------------------------------------------------------------------------------------------------
// A head is the first record of a run of equal slots: TileHeadPred<u32> over the sorted slots, counted and ranked per record tile by
// tile_rank.h.

// segment g starts at seg_start[g]; seg_start[segments] = n.  seg_start has n + 1 entries, segments <= n is read from the scan's total.
__global__ __launch_bounds__(LB_T) void k_lb_heads(const u32 * __restrict__ ss, u64 n, u64 n_tiles, const u64 * __restrict__ tile_off, const u64 * __restrict__ segments,
                                                   u32 * __restrict__ seg_start)
{
    __shared__ u32 s_wave[LB_T / 64];
    if (blockIdx.x == 0 && threadIdx.x == 0 && *segments <= n)
        seg_start[*segments] = (u32)n;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    {
        u64 m[TILE_R];
        const u64 pos = tile_off[tile] + tile_ballots(TileHeadPred<u32>{ss}, tile, n, m, s_wave);
        tile_for_ranked(m, tile, pos, [&](u64 i, u64 g) {
            if (g < n)
                seg_start[g] = (u32)i;
        });
        __syncthreads();
    }
}

// every record's rank in its segment and whether its row passes; the counters are only read here
__global__ __launch_bounds__(LB_T) void k_lb_rank_apply(const u32 * __restrict__ ss, const u32 * __restrict__ sr, u64 n_live, u64 n_tiles, const u64 * __restrict__ tile_off,
                                                        const u32 * __restrict__ seg_start, const u32 * __restrict__ count, u32 offset, u32 bound, u8 * __restrict__ filter,
                                                        u64 n, LbCtl * ctl)
{
    __shared__ u32 s_wave[LB_T / 64];
    u32 passed = 0;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    {
        u64 m[TILE_R];
        u64 pos = tile_off[tile] + tile_ballots(TileHeadPred<u32>{ss}, tile, n_live, m, s_wave);
#pragma unroll
        for (u32 r = 0; r < TILE_R; ++r)
        {
            const u64 i = tile_item(tile, r);
            // heads at or before this record, over the whole input: its segment is that number - 1
            const u64 upto = pos + mbcnt(m[r]) + ((m[r] >> lane_id()) & 1);
            if (i < n_live && upto >= 1 && upto <= n_live)
            {
                const u32 head = seg_start[upto - 1];
                const u32 row = sr[i];
                const u64 k = (u64)count[ss[i]] + (i - head);
                const bool pass = head <= i && k >= offset && k < bound;
                if (row < n)
                    filter[row] = pass;
                passed += pass;
            }
            pos += (u32)__popcll(m[r]);
        }
        __syncthreads();
    }
    lb_fold_count(passed, &ctl->passed);
}

// one lane per segment raises its slot's counter by the segment's length, up to offset + length
__global__ __launch_bounds__(LB_T) void k_lb_count_update(const u32 * __restrict__ ss, const u32 * __restrict__ seg_start, const u64 * __restrict__ segments, u64 n_live,
                                                          u32 * __restrict__ count, u32 bound, LbCtl * ctl)
{
    const u64 G = *segments <= n_live ? *segments : 0;
    u32 counted = 0;
    for (u64 g = (u64)blockIdx.x * LB_T + threadIdx.x; g < G; g += (u64)gridDim.x * LB_T)
    {
        const u32 a = seg_start[g], b = seg_start[g + 1];
        if (a < b && b <= n_live)
        {
            const u32 slot = ss[a];
            const u32 c = count[slot];
            const u64 next = (u64)c + (b - a);
            count[slot] = next < bound ? (u32)next : bound;
            counted += c == 0;
        }
    }
    lb_fold_count(counted, &ctl->counted);
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static constexpr PairNames LB_NAMES{"limit_by", "operator", "an operator"};

struct chgpu_limit_by : PairOp
{
    u32 offset = 0, bound = 0; // group_offset, group_offset + group_length
    u64 cap = 0;
    u64 occupied = 0; // cells taken (keys of a failed call included)
    u64 counted = 0;  // counters > 0
    PairMem cells, count, claim, ctl;
    PairAllocs mem;
};

static u32 lb_grid(chgpu_ctx * ctx, u64 blocks_wanted)
{
    const long long forced = chgpu_opt(ctx, "test_limit_by_grid", 0);
    if (forced > 0)
        return (u32)(forced < 65536 ? forced : 65536);
    return chgpu_grid_for(ctx, blocks_wanted, 1, 8);
}

static int lb_ctl_reset(chgpu_limit_by * d)
{
    CHGPU_HIP(hipMemsetAsync(d->ctl.p, 0, sizeof(LbCtl), d->ctx->stream));
    return CHGPU_OK;
}

static int lb_ctl_read(chgpu_limit_by * d, LbCtl * host) { return chgpu_read_back(d->ctx, d->ctl.p, host, sizeof(LbCtl)); }

// a cleared table of `cap` cells: every allocation first
static int lb_new_table(chgpu_limit_by * d, u64 cap, PairMem * cells, PairMem * count, PairMem * claim)
{
    chgpu_ctx * ctx = d->ctx;
    int rc = d->mem.alloc(cap * 8, cells);
    if (rc == CHGPU_OK)
        rc = d->mem.alloc((cap + 1) * 4, count);
    if (rc == CHGPU_OK)
        rc = d->mem.alloc((cap + 1) * 4, claim);
    if (rc == CHGPU_OK &&
        (hipMemsetAsync(cells->p, 0, cap * 8, ctx->stream) != hipSuccess || hipMemsetAsync(count->p, 0, (cap + 1) * 4, ctx->stream) != hipSuccess ||
         hipMemsetAsync(claim->p, 0xFF, (cap + 1) * 4, ctx->stream) != hipSuccess))
        rc = chgpu_set_error(CHGPU_ERR_DEVICE, "limit_by: clearing the table failed");
    if (rc != CHGPU_OK)
    {
        pair_free_mem(ctx, *cells);
        pair_free_mem(ctx, *count);
        pair_free_mem(ctx, *claim);
    }
    return rc;
}

// the table into one of `cap` cells, keys and counters together
static int lb_grow_to(chgpu_limit_by * d, u64 cap)
{
    chgpu_ctx * ctx = d->ctx;
    PairMem cells, count, claim;
    CHGPU_TRY(lb_new_table(d, cap, &cells, &count, &claim));
    hipLaunchKernelGGL(k_lb_rehash, dim3(chgpu_grid_for(ctx, d->cap, LB_T, 8)), dim3(LB_T), 0, ctx->stream, (const u64 *)d->cells.p, (const u32 *)d->count.p, d->cap,
                       (u64 *)cells.p, (u32 *)count.p, cap);
    ctx->counters[6] += 1;
    pair_free_mem(ctx, d->cells); // reuse is ordered behind the rehash (same stream)
    pair_free_mem(ctx, d->count);
    pair_free_mem(ctx, d->claim);
    d->cells = cells;
    d->count = count;
    d->claim = claim;
    d->cap = cap;
    return pair_launch_ok(LB_NAMES, "rehash");
}

extern "C" int chgpu_limit_by_create(chgpu_ctx * ctx, int key_type, uint64_t group_length, uint64_t group_offset, uint64_t size_hint, chgpu_limit_by ** out)
{
    CHGPU_REQUIRE(ctx && out, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(key_type >= 0, CHGPU_ERR_NOT_IMPLEMENTED, "limit_by: without a key the clause is a plain LIMIT");
    CHGPU_REQUIRE(chgpu_type_size(key_type) != 0, CHGPU_ERR_BAD_ARGUMENTS, "limit_by: unknown key type %d", key_type);
    CHGPU_REQUIRE(chgpu_type_is_int(key_type), CHGPU_ERR_NOT_IMPLEMENTED, "limit_by: key type %d: integer keys only (CPU path)", key_type);
    const char * msg = "";
    const int code = lb_check_bounds(group_length, group_offset, &msg);
    CHGPU_REQUIRE(code == CHGPU_OK, code, "limit_by: %s", msg);
    const u64 cap = lb_capacity_for(size_hint);
    CHGPU_REQUIRE(cap != 0, CHGPU_ERR_TOO_MANY_ROWS, "limit_by: size_hint %llu, at most %llu keys fit", (unsigned long long)size_hint, (unsigned long long)LB_MAX_KEYS);
    ChgpuDeviceGuard guard(ctx);
    chgpu_limit_by * d = new chgpu_limit_by();
    d->ctx = ctx;
    d->key_type = key_type;
    d->mem = PairAllocs{ctx, LB_NAMES.op, "test_limit_by_fail_alloc"};
    d->offset = (u32)group_offset;
    d->bound = (u32)(group_offset + group_length);
    chgpu_ctx_retain(ctx);
    int rc = chgpu_pool_alloc(ctx, sizeof(LbCtl), &d->ctl.p, &d->ctl.cls);
    if (rc == CHGPU_OK)
        rc = lb_new_table(d, cap, &d->cells, &d->count, &d->claim);
    if (rc != CHGPU_OK)
    {
        chgpu_limit_by_free(d);
        return rc;
    }
    d->cap = cap;
    *out = d;
    return CHGPU_OK;
}

extern "C" int chgpu_limit_by_free(chgpu_limit_by * d)
{
    if (!d)
        return CHGPU_OK;
    ChgpuDeviceGuard guard(d->ctx);
    pair_free_mem(d->ctx, d->cells);
    pair_free_mem(d->ctx, d->count);
    pair_free_mem(d->ctx, d->claim);
    pair_free_mem(d->ctx, d->ctl);
    chgpu_ctx * ctx = d->ctx;
    delete d;
    chgpu_ctx_release(ctx);
    return CHGPU_OK;
}

extern "C" int chgpu_limit_by_keys(chgpu_limit_by * d, uint64_t * keys)
{
    CHGPU_REQUIRE(d && keys, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    *keys = d->counted;
    return CHGPU_OK;
}

// what a block's kernels share
struct LbBlock
{
    const void * kp; // the range's first key
    const u8 * fp;   // its first filter byte, or NULL
    u32 key_size, lead;
    u64 n, vn, n_tiles;
    u32 * slot;
    u32 * tile_counts;
};

static void lb_launch_resolve(chgpu_limit_by * d, const LbBlock & b)
{
    chgpu_ctx * ctx = d->ctx;
    dispatch_width(b.key_size, [&](auto tag) {
        typedef decltype(tag) K;
        hipLaunchKernelGGL(k_lb_resolve<K>, dim3(lb_grid(ctx, b.n_tiles)), dim3(LB_T), 0, ctx->stream, (const K *)b.kp, b.fp, b.lead, b.vn, b.n_tiles, (const u64 *)d->cells.p,
                           d->cap, (const u32 *)d->count.p, d->bound, b.slot, b.tile_counts, (LbCtl *)d->ctl.p);
    });
    ctx->counters[6] += 1;
}

static void lb_launch_insert(chgpu_limit_by * d, const LbBlock & b, u32 room)
{
    chgpu_ctx * ctx = d->ctx;
    dispatch_width(b.key_size, [&](auto tag) {
        typedef decltype(tag) K;
        hipLaunchKernelGGL(k_lb_insert<K>, dim3(lb_grid(ctx, (b.vn + LB_T - 1) / LB_T)), dim3(LB_T), 0, ctx->stream, (const K *)b.kp, b.lead, b.vn, (const u32 *)b.slot,
                           (u64 *)d->cells.p, d->cap, room, (LbCtl *)d->ctl.p);
    });
    ctx->counters[6] += 1;
}

// Every row of the block gets its slot.  Resolve; while rows are missing: an insert round over them (into a larger table when
// lb_should_grow says so: the round before met the limit with the table at least half way there), then resolve again over the table as
// it then stands.  A round that met the limit only because rows of few new keys asked together does not make the table grow.  *seen: the totals of
// the last resolve.
static int lb_resolve_all(chgpu_limit_by * d, const LbBlock & b, LbCtl * seen, LbPlan * plan)
{
    bool limit_met = false;
    u32 stalled = 0; // rounds in a row that met the limit on this table far below it
    for (u32 rounds = 0;; ++rounds)
    {
        CHGPU_TRY(lb_ctl_reset(d));
        lb_launch_resolve(d, b);
        CHGPU_TRY(pair_launch_ok(LB_NAMES, "resolve"));
        CHGPU_TRY(lb_ctl_read(d, seen));
        CHGPU_REQUIRE(seen->live <= seen->entered && seen->entered <= b.n && seen->missing <= seen->live, CHGPU_ERR_LOGICAL, "limit_by: %u live of %u entered of %llu rows",
                      seen->live, seen->entered, (unsigned long long)b.n);
        if (seen->missing == 0)
            return CHGPU_OK;
        CHGPU_REQUIRE(rounds < 64, CHGPU_ERR_LOGICAL, "limit_by: %u rows without a slot after %u insert rounds", seen->missing, rounds);
        if (lb_should_grow(d->cap, d->occupied, limit_met, stalled))
        {
            stalled = 0;
            const u64 next = lb_next_capacity(d->cap, d->occupied, seen->missing);
            CHGPU_REQUIRE(next != 0, CHGPU_ERR_TOO_MANY_ROWS, "limit_by: more than %llu keys", (unsigned long long)LB_MAX_KEYS);
            CHGPU_TRY(lb_grow_to(d, next));
            plan->grown += 1;
        }
        else if (limit_met)
            stalled += 1;
        const u64 room = lb_limit(d->cap) - d->occupied;
        LbCtl round{};
        CHGPU_TRY(lb_ctl_reset(d));
        lb_launch_insert(d, b, (u32)(room < 0xFFFFFFFFull ? room : 0xFFFFFFFFull));
        CHGPU_TRY(pair_launch_ok(LB_NAMES, "insert"));
        CHGPU_TRY(lb_ctl_read(d, &round));
        CHGPU_REQUIRE(round.inserted <= room, CHGPU_ERR_LOGICAL, "limit_by: %u keys inserted into room for %llu", round.inserted, (unsigned long long)room);
        d->occupied += round.inserted;
        limit_met = round.overflow != 0;
        CHGPU_REQUIRE(limit_met || round.inserted != 0, CHGPU_ERR_LOGICAL, "limit_by: %u rows without a slot and nothing to insert", seen->missing);
    }
}

static int lb_filter_block(chgpu_limit_by * d, const chgpu_col * key_col, u64 row_begin, u64 n, const chgpu_col * filter_u8, chgpu_col * out, LbPlan * plan)
{
    chgpu_ctx * ctx = d->ctx;
    PairTemps tmp(d->mem);
    LbBlock b{};
    b.key_size = (u32)chgpu_type_size(d->key_type);
    b.kp = (const char *)key_col->data + row_begin * b.key_size;
    b.fp = filter_u8 ? (const u8 *)filter_u8->data + row_begin : nullptr;
    b.lead = (u32)(((uintptr_t)b.kp / b.key_size) & (LB_V - 1));
    b.n = n;
    b.vn = n + b.lead;
    b.n_tiles = (b.vn + LB_TILE - 1) / LB_TILE;
    u64 * tile_off = nullptr; // [n_tiles], then the total
    CHGPU_TRY(tmp.alloc(b.n_tiles * LB_TILE * 4, (void **)&b.slot));
    CHGPU_TRY(tmp.alloc(b.n_tiles * 4, (void **)&b.tile_counts));
    CHGPU_TRY(tmp.alloc((b.n_tiles + 1) * 8, (void **)&tile_off));
    CHGPU_HIP(hipMemsetAsync(out->data, 0, n, ctx->stream)); // dead rows, and every row until a plan says otherwise

    LbCtl seen{};
    CHGPU_TRY(lb_resolve_all(d, b, &seen, plan));
    plan->entered = seen.entered;
    plan->live = seen.live;
    plan->kind = lb_choose_plan(seen.live, d->bound);
    if (plan->kind == LB_PLAN_DEAD)
        return CHGPU_OK;

    // the live rows as (slot, row) records in row order
    const u64 L = seen.live;
    chgpu_col * rec_slot = nullptr;
    chgpu_col * rec_row = nullptr;
    CHGPU_TRY(tmp.col(CHGPU_U32, L, &rec_slot));
    CHGPU_TRY(tmp.col(CHGPU_U32, L, &rec_row));
    const u64 rec_tiles = (L + LB_RTILE - 1) / LB_RTILE;
    u32 * head_counts = nullptr;
    u64 * head_off = nullptr; // [rec_tiles], then the number of segments
    u32 * seg_start = nullptr;
    u32 shifts[4];
    if (plan->kind == LB_PLAN_RANK)
    {
        plan->passes = lb_plan_passes(seen.or_bits, ~seen.nand_bits, shifts);
        CHGPU_TRY(tmp.alloc(rec_tiles * 4, (void **)&head_counts));
        CHGPU_TRY(tmp.alloc((rec_tiles + 1) * 8, (void **)&head_off));
        CHGPU_TRY(tmp.alloc((L + 1) * 4, (void **)&seg_start));
    }
    CHGPU_TRY(tile_scan(ctx, b.tile_counts, tile_off, b.n_tiles, tile_off + b.n_tiles));
    hipLaunchKernelGGL(k_lb_compact, dim3(lb_grid(ctx, b.n_tiles)), dim3(LB_T), 0, ctx->stream, (const u32 *)b.slot, b.lead, b.n_tiles, (const u64 *)tile_off, L,
                       (u32 *)rec_slot->data, (u32 *)rec_row->data);
    ctx->counters[6] += 1;
    CHGPU_TRY(pair_launch_ok(LB_NAMES, "compact"));

    const chgpu_col * cur[2] = {rec_slot, rec_row};
    const size_t own = tmp.cols.size(); // the latest pass's two columns, freed with the call like the records
    tmp.cols.resize(own + 2, nullptr);
    CHGPU_TRY(pair_run_passes(d->mem, shifts, plan->passes, cur, &tmp.cols[own]));
    // from here on nothing is allocated: counters and claims change
    CHGPU_TRY(lb_ctl_reset(d));
    const u32 * ss = (const u32 *)cur[0]->data;
    const u32 * sr = (const u32 *)cur[1]->data;
    const dim3 block(LB_T), tgrid(lb_grid(ctx, rec_tiles));
    if (plan->kind == LB_PLAN_CLAIM)
    {
        hipLaunchKernelGGL(k_lb_claim_min, tgrid, block, 0, ctx->stream, ss, sr, L, rec_tiles, (u32 *)d->claim.p);
        hipLaunchKernelGGL(k_lb_claim_pass, dim3(lb_grid(ctx, (L + LB_T - 1) / LB_T)), block, 0, ctx->stream, ss, sr, L, (u32 *)d->claim.p, (u32 *)d->count.p,
                           (u8 *)out->data, n, (LbCtl *)d->ctl.p);
        ctx->counters[6] += 2;
    }
    else
    {
        hipLaunchKernelGGL(k_tile_counts<TileHeadPred<u32>>, tgrid, block, 0, ctx->stream, TileHeadPred<u32>{ss}, L, rec_tiles, head_counts);
        CHGPU_TRY(tile_scan(ctx, head_counts, head_off, rec_tiles, head_off + rec_tiles));
        const u64 * segments = head_off + rec_tiles;
        hipLaunchKernelGGL(k_lb_heads, tgrid, block, 0, ctx->stream, ss, L, rec_tiles, (const u64 *)head_off, segments, seg_start);
        hipLaunchKernelGGL(k_lb_rank_apply, tgrid, block, 0, ctx->stream, ss, sr, L, rec_tiles, (const u64 *)head_off, (const u32 *)seg_start, (const u32 *)d->count.p,
                           d->offset, d->bound, (u8 *)out->data, n, (LbCtl *)d->ctl.p);
        hipLaunchKernelGGL(k_lb_count_update, dim3(lb_grid(ctx, (L + LB_T - 1) / LB_T)), block, 0, ctx->stream, ss, (const u32 *)seg_start, segments, L, (u32 *)d->count.p,
                           d->bound, (LbCtl *)d->ctl.p);
        ctx->counters[6] += 4;
    }
    CHGPU_TRY(pair_launch_ok(LB_NAMES, "apply"));
    LbCtl done{};
    CHGPU_TRY(lb_ctl_read(d, &done)); // the one read for rows_passed
    plan->passed = done.passed;
    d->counted += plan->kind == LB_PLAN_CLAIM ? done.passed : done.counted;
    return CHGPU_OK;
}

extern "C" int chgpu_limit_by_filter_block(chgpu_limit_by * d, const chgpu_col * key_col, uint64_t row_begin, uint64_t row_end, const chgpu_col * filter_u8,
                                           chgpu_col ** out_filter_u8, uint64_t * rows_passed)
{
    CHGPU_REQUIRE(d && key_col && out_filter_u8 && rows_passed, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(key_col->type == d->key_type, CHGPU_ERR_BAD_ARGUMENTS, "limit_by: key column of type %d, the operator was made for %d", key_col->type, d->key_type);
    CHGPU_REQUIRE(!filter_u8 || filter_u8->type == CHGPU_U8, CHGPU_ERR_BAD_ARGUMENTS, "limit_by: the filter must be UInt8");
    CHGPU_TRY(pair_check_device(LB_NAMES, *d, key_col, filter_u8));
    const char * msg = "";
    const int code = lb_check_rows(key_col->rows, filter_u8 ? (int64_t)filter_u8->rows : -1, row_begin, row_end, &msg);
    CHGPU_REQUIRE(code == CHGPU_OK, code, "limit_by: %s", msg);
    chgpu_ctx * ctx = d->ctx;
    ChgpuDeviceGuard guard(ctx);
    d->mem.begin_call();
    const u64 n = row_end - row_begin;
    LbPlan plan;
    plan.n = n;
    plan.keys_before = plan.keys = d->counted;
    plan.cap_before = plan.cap = d->cap;
    chgpu_col * out = nullptr;
    int rc = d->mem.col_new(CHGPU_U8, n, &out);
    if (rc == CHGPU_OK && n)
        rc = lb_filter_block(d, key_col, row_begin, n, filter_u8, out, &plan);
    plan.keys = d->counted;
    plan.cap = d->cap;
    plan.rc = rc;
    pair_print_plan(ctx, lb_format_plan, plan);
    if (rc != CHGPU_OK)
    {
        if (out) chgpu_col_free(out);
        return rc;
    }
    *out_filter_u8 = out;
    *rows_passed = plan.passed;
    return CHGPU_OK;
}
