#!/usr/bin/env python3
"""Cost of conditioned aggregates (-If / Nullable arguments): UInt64 keys, Int64 values, a table that already holds
every key.
  (a) sum(v), count()                                   no conditions: the existing caller
  (b) sumIf(v, c), countIf(c)                            50 % kept
  (c) sumIf(v, c1), sumIf(v, c2), countIf(c1), count()   50 % and 10 % kept
  (d) what a caller could do before: one WHERE-filtered aggregator per distinct condition over the same rows (c1: sum, count; c2: sum;
      none: count).  It answers a weaker question (a group whose rows all fail is lost); it is the cost baseline of (c).
Every case is warmed up once and timed with device events over enough repetitions to fill well over 0.1 s; the plan is the one the
size hint (= groups) selects and is reported beside the time.
usage: python tools/bench_agg_conditions.py [rows,rows...] [groups,groups...] [out.json]  -> one JSON line (and the file)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clickhouse_amd as ch

rows_list = [int(float(x)) for x in (sys.argv[1] if len(sys.argv) > 1 else "1e8,1e9").split(",")]
groups_list = [int(float(x)) for x in (sys.argv[2] if len(sys.argv) > 2 else "1000,1e6").split(",")]
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r04_agg_conditions.json")
dev = torch.device("cuda:0")
ctx = ch.Context(0)
MULT = 2654435761


def timed(fn):
    """ms per call: one warm-up, then repetitions until well over 0.1 s of device time"""
    fn()
    ctx.timer_start()
    fn()
    one = max(ctx.timer_stop_ms(), 1e-3)
    reps = max(3, int(250.0 / one) + 1)
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return round(ctx.timer_stop_ms() / reps, 3), reps


out = {"metric": "ms per block, device events, mean over reps", "cases": []}
for rows in rows_list:
    g = torch.Generator(device=dev).manual_seed(5)
    gid = torch.randint(0, max(groups_list), (rows,), dtype=torch.int64, device=dev, generator=g)
    v = torch.randint(-2**40, 2**40, (rows,), dtype=torch.int64, device=dev, generator=g)
    c1 = (torch.rand(rows, device=dev, generator=g) < 0.5).to(torch.uint8)
    c2 = (torch.rand(rows, device=dev, generator=g) < 0.1).to(torch.uint8)
    vc = ctx.wrap(v.data_ptr(), np.int64, rows, keepalive=v)
    c1c = ctx.wrap(c1.data_ptr(), np.uint8, rows, keepalive=c1)
    c2c = ctx.wrap(c2.data_ptr(), np.uint8, rows, keepalive=c2)
    for groups in groups_list:
        keys = (gid % groups) * MULT + 17
        every = torch.arange(groups, dtype=torch.int64, device=dev) * MULT + 17
        kc = ctx.wrap(keys.data_ptr(), np.uint64, rows, keepalive=keys)
        ec = ctx.wrap(every.data_ptr(), np.uint64, groups, keepalive=every)
        zeros = torch.zeros(groups, dtype=torch.int64, device=dev)
        ones = torch.ones(groups, dtype=torch.uint8, device=dev)
        ev = ctx.wrap(zeros.data_ptr(), np.int64, groups, keepalive=zeros)
        eo = ctx.wrap(ones.data_ptr(), np.uint8, groups, keepalive=ones)
        torch.cuda.synchronize()   # the inputs come from torch's stream; the library reads them on its own
        res = {"rows": rows, "groups": groups}

        def make(aggs):
            ag = ch.Aggregator(np.uint64, aggs, size_hint=groups, ctx=ctx)
            ag.execute_on_block(ec, [None if k == ch.AGG_COUNT else ev for k, *_ in aggs], conds=[eo if len(e) > 2 else None for e in aggs] if any(len(e) > 2 for e in aggs) else None)
            return ag

        A = make([(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)])
        res["a_ms"], res["a_reps"] = timed(lambda: A.execute_on_block(kc, [vc, None]))
        B = make([(ch.AGG_SUM, np.int64, "if"), (ch.AGG_COUNT, None, "if")])
        res["b_ms"], _ = timed(lambda: B.execute_on_block(kc, [vc, None], conds=[c1c, c1c]))
        Cc = make([(ch.AGG_SUM, np.int64, "if"), (ch.AGG_SUM, np.int64, "if"), (ch.AGG_COUNT, None, "if"), (ch.AGG_COUNT, None)])
        res["c_ms"], _ = timed(lambda: Cc.execute_on_block(kc, [vc, vc, None, None], conds=[c1c, c2c, c1c, None]))
        D1 = make([(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)])
        D2 = make([(ch.AGG_SUM, np.int64)])
        D3 = make([(ch.AGG_COUNT, None)])

        def d_run():
            D1.execute_on_block(kc, [vc, None], filter=c1c)
            D2.execute_on_block(kc, [vc], filter=c2c)
            D3.execute_on_block(kc, [None])

        res["d_ms"], _ = timed(d_run)
        assert len(A) == len(B) == len(Cc) == groups, res
        # (b) against torch: countIf over all calls = the priming block's one row per group + a whole number of blocks' kept rows
        kept = int(c1.sum().item())
        _, rb = B.convert_to_block()
        total = int(rb[1].sum()) - groups
        assert total > 0 and total % kept == 0, (total, kept)
        res["b_over_a"] = round(res["b_ms"] / res["a_ms"], 3)
        res["c_over_a"] = round(res["c_ms"] / res["a_ms"], 3)
        res["c_over_d"] = round(res["c_ms"] / res["d_ms"], 3)
        out["cases"].append(res)
        print(json.dumps(res), file=sys.stderr, flush=True)
        for x in (A, B, Cc, D1, D2, D3):
            x.close()
        del keys, kc
print(json.dumps(out))
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
