#!/usr/bin/env python3
"""Cost of the argMin / argMax passes: UInt64 key, Int64 val, Int64 arg, one block.
  (a) max(val), any(arg)   -- the DIRECT kernel + k_agg_any_resolve: two passes that probe the table
  (b) argMax(arg, val)     -- the DIRECT kernel + the claim pass + the resolve pass: three
Both touch the same columns and, per group, words combined the same way ({order key} + {claim, value} against {val key, claim, arg}).
Each case aggregates the block into a fresh table (size hint = groups), best of 3.
usage: python tools/bench_arg_min_max.py [rows] [groups,groups...] [out.json]  -> one JSON line (also written to out.json)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clickhouse_amd as ch

rows = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
groups_list = [int(float(x)) for x in (sys.argv[2] if len(sys.argv) > 2 else "1000,1e6").split(",")]
out_path = sys.argv[3] if len(sys.argv) > 3 else None
dev = torch.device("cuda:0")
ctx = ch.Context(0)
MULT = 2654435761

g = torch.Generator(device=dev).manual_seed(5)
gid = torch.randint(0, max(groups_list), (rows,), dtype=torch.int64, device=dev, generator=g)
val = torch.randint(-2**40, 2**40, (rows,), dtype=torch.int64, device=dev, generator=g)
arg = torch.arange(rows, dtype=torch.int64, device=dev)
vc = ctx.wrap(val.data_ptr(), np.int64, rows, keepalive=val)
ac = ctx.wrap(arg.data_ptr(), np.int64, rows, keepalive=arg)


def timed(make, feed):
    best = 1e9
    for _ in range(3):
        ag = make()
        ctx.synchronize()
        t0 = time.perf_counter()
        feed(ag)
        ctx.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
        n = len(ag)
        ag.close()
    return round(best, 3), n


out = {"metric": "ms per block into a fresh table, best of 3", "rows": rows, "cases": []}
for groups in groups_list:
    keys = (gid % groups) * MULT + 17
    kc = ctx.wrap(keys.data_ptr(), np.uint64, rows, keepalive=keys)
    torch.cuda.synchronize()  # the inputs come from torch's stream; the library reads them on its own
    res = {"rows": rows, "groups": groups}
    res["max_any_ms"], n1 = timed(lambda: ch.Aggregator(np.uint64, [(ch.AGG_MAX, np.int64), (ch.AGG_ANY, np.int64)], size_hint=groups, ctx=ctx),
                                  lambda ag: ag.execute_on_block(kc, [vc, ac]))
    res["arg_max_ms"], n2 = timed(lambda: ch.Aggregator(np.uint64, [(ch.AGG_ARG_MAX, (np.int64, np.int64))], size_hint=groups, ctx=ctx),
                                  lambda ag: ag.execute_on_block(kc, [(ac, vc)]))
    assert n1 == n2 == groups, (n1, n2, groups)
    res["arg_max_over_max_any"] = round(res["arg_max_ms"] / res["max_any_ms"], 3)
    # the winner is a row of its group that holds the group's maximum (arg is the row number)
    ag = ch.Aggregator(np.uint64, [(ch.AGG_ARG_MAX, (np.int64, np.int64)), (ch.AGG_MAX, np.int64)], size_hint=groups, ctx=ctx)
    ag.execute_on_block(kc, [(ac, vc), vc])
    gk, (win, mx) = ag.convert_to_block()
    w = torch.from_numpy(win).to(dev)
    assert torch.equal(val[w].cpu(), torch.from_numpy(mx)) and torch.equal(keys[w].cpu().view(torch.int64), torch.from_numpy(gk.view(np.int64)))
    ag.close()
    out["cases"].append(res)
    print(json.dumps(res), file=sys.stderr, flush=True)
    del keys, kc
line = json.dumps(out)
if out_path:
    with open(out_path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
print(line)
