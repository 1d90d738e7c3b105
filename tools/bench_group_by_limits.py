#!/usr/bin/env python3
"""Cost of the find-only (no_more_keys) GROUP BY path: UInt64 keys, sum(Int64) + count(), a table that already holds every key.
  (a) the ordinary add of the block (chgpu_agg_add_block)
  (b) the same block find-only (max_rows_to_group_by crossed under ANY: chgpu_agg_execute_on_block with no_more_keys)
  (c) find-only with half the rows' keys absent, the overflow row on (they go to it)
Best of 3 per case; the plan is the one the size hint (= groups) selects, the same for all three.
usage: python tools/bench_group_by_limits.py [rows,rows...] [groups,groups...]  -> one JSON line"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clickhouse_amd as ch

rows_list = [int(float(x)) for x in (sys.argv[1] if len(sys.argv) > 1 else "1e8,1e9").split(",")]
groups_list = [int(float(x)) for x in (sys.argv[2] if len(sys.argv) > 2 else "1000,1e6").split(",")]
dev = torch.device("cuda:0")
ctx = ch.Context(0)
aggs = [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)]
MULT = 2654435761


def timed(fn):
    best = 1e9
    for _ in range(3):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return round(best, 3)


out = {"metric": "ms per block, best of 3", "cases": []}
for rows in rows_list:
    g = torch.Generator(device=dev).manual_seed(5)
    gid = torch.randint(0, max(groups_list), (rows,), dtype=torch.int64, device=dev, generator=g)
    v = torch.randint(-2**40, 2**40, (rows,), dtype=torch.int64, device=dev, generator=g)
    half = torch.rand(rows, device=dev, generator=g) < 0.5
    vc = ctx.wrap(v.data_ptr(), np.int64, rows, keepalive=v)
    for groups in groups_list:
        keys = (gid % groups) * MULT + 17
        keys_half = torch.where(half, keys, keys + groups * MULT)     # half the rows: a key no block 1 had
        every = torch.arange(groups, dtype=torch.int64, device=dev) * MULT + 17
        kc = ctx.wrap(keys.data_ptr(), np.uint64, rows, keepalive=keys)
        khc = ctx.wrap(keys_half.data_ptr(), np.uint64, rows, keepalive=keys_half)
        ec = ctx.wrap(every.data_ptr(), np.uint64, groups, keepalive=every)
        ev_keep = torch.zeros(groups, dtype=torch.int64, device=dev)
        ev = ctx.wrap(ev_keep.data_ptr(), np.int64, groups, keepalive=ev_keep)
        torch.cuda.synchronize()   # the inputs come from torch's stream; the library reads them on its own
        res = {"rows": rows, "groups": groups}
        A = ch.Aggregator(np.uint64, aggs, size_hint=groups, ctx=ctx)
        A.execute_on_block(ec, [ev, None])
        res["a_add_ms"] = timed(lambda: A.execute_on_block(kc, [vc, None]))
        B = ch.Aggregator(np.uint64, aggs, size_hint=groups, ctx=ctx, max_rows_to_group_by=groups - 1, group_by_overflow_mode="any")
        B.execute_on_block(ec, [ev, None])
        assert B.no_more_keys
        res["b_find_only_ms"] = timed(lambda: B.execute_on_block(kc, [vc, None]))
        C = ch.Aggregator(np.uint64, aggs, size_hint=groups, ctx=ctx, max_rows_to_group_by=groups - 1, group_by_overflow_mode="any",
                          overflow_row=True)
        C.execute_on_block(ec, [ev, None])
        res["c_find_only_half_missing_ms"] = timed(lambda: C.execute_on_block(khc, [vc, None]))
        res["groups_after"] = [len(A), len(B), len(C)]
        assert len(A) == len(B) == len(C) == groups, res
        o = C.overflow_row()
        missing = int((~half).sum().item())
        assert int(o[1].numpy()[0]) == 3 * missing, (int(o[1].numpy()[0]), missing)
        res["b_over_a"] = round(res["b_find_only_ms"] / res["a_add_ms"], 3)
        res["c_over_a"] = round(res["c_find_only_half_missing_ms"] / res["a_add_ms"], 3)
        out["cases"].append(res)
        print(json.dumps(res), file=sys.stderr, flush=True)
        for x in (A, B, C):
            x.close()
        del keys, keys_half, kc, khc
print(json.dumps(out))
