#!/usr/bin/env python3
"""Substring search over a URL-like ColumnString on one MI355X: GB/s of `chars` per call, HIP-event timed on the context's stream.
  (a) contains(needle) down the flat kernel, for a needle in about 1 % of the rows ("google") and one in every row ("http")
  (b) the yardstick: a read-only stream of the same bytes with the library's own streaming reader (chgpu_count_bytes_in_filter over chars)
  (c) the same two needles as %needle% down the general per-row matcher (developer option tune_str_contains_general)
Every value is "http://" + 32..112 random bytes of [a-z./-_=0]; one row in a hundred carries "google".  A call is what a caller pays:
the offsets check, the mask pre-fill, the tile pre-pass and the search.  The masks of (a) and (c) must be equal and hit the planted rows.
usage: python tools/bench_string_match.py [--gib 1.0] [--reps 10] [--warmup 3] [--commit ID] [--out FILE]  -> one JSON line"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clickhouse_amd as ch

ap = argparse.ArgumentParser()
ap.add_argument("--gib", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

dev = torch.device("cuda:0")
ctx = ch.Context(0)
g = torch.Generator(device=dev).manual_seed(17)
rows = int(args.gib * 2**30 / 80)
lens = torch.randint(40, 121, (rows,), dtype=torch.int64, device=dev, generator=g)        # value bytes, "http://" included; mean 80
offsets = torch.cumsum(lens + 1, 0)                                                        # int64 bits = the UInt64 offsets
size = int(offsets[-1].item())
begins = offsets - lens - 1
table = torch.tensor(list(b"abcdefghijklmnopqrstuvwxyz./-_=0"), dtype=torch.uint8, device=dev)
chars = torch.empty(size + 64, dtype=torch.uint8, device=dev)                              # + the pad a wrapped chars column needs
STEP = 1 << 26
for lo in range(0, size, STEP):
    n = min(STEP, size - lo)
    chars[lo:lo + n] = table[torch.randint(0, 32, (n,), dtype=torch.int64, device=dev, generator=g)]
chars[size:] = 0
for k, b in enumerate(b"http://"):
    chars[begins + k] = b
planted = torch.arange(0, rows, 100, device=dev)
for k, b in enumerate(b"google"):
    chars[begins[planted] + 12 + k] = b
chars[offsets - 1] = 0
torch.cuda.synchronize()      # the inputs come from torch's stream; the library reads them on its own
col = ch.ColumnString(ctx.wrap(offsets.data_ptr(), np.uint64, rows, keepalive=offsets), ctx.wrap(chars.data_ptr(), np.uint8, size, keepalive=chars))


def timed(fn):
    for _ in range(args.warmup):
        fn()
    ctx.timer_start()
    for _ in range(args.reps):
        fn()
    return ctx.timer_stop_ms() / args.reps


def rate(ms):
    return round(size / ms / 1e6, 1)      # GB/s of chars


res = {"tool": "tools/bench_string_match.py", "commit": args.commit, "rows": rows, "chars_bytes": size, "mean_value_bytes": round(size / rows - 1, 2),
       "metric": "GB/s of chars per call (HIP events, mean of %d calls after %d warm-up calls)" % (args.reps, args.warmup)}
masks = {}
for name, needle in (("1pct", b"google"), ("every_row", b"http")):
    ms = timed(lambda: col.contains(needle))
    masks[name] = col.contains(needle)
    hits = ch.count_bytes_in_filter(masks[name])
    res["a_flat_" + name] = {"needle": needle.decode(), "ms": round(ms, 4), "GBps": rate(ms), "rows_hit": hits}
    print(json.dumps({name: res["a_flat_" + name]}), file=sys.stderr, flush=True)
assert res["a_flat_every_row"]["rows_hit"] == rows, res
assert abs(res["a_flat_1pct"]["rows_hit"] - (rows + 99) // 100) <= 64, res       # the planted rows, and the odd random "google"
ms = timed(lambda: ch.count_bytes_in_filter(col.chars))
res["b_stream_read"] = {"what": "chgpu_count_bytes_in_filter over chars", "ms": round(ms, 4), "GBps": rate(ms)}
ctx.set_option("tune_str_contains_general", 1)
for name, needle in (("1pct", b"google"), ("every_row", b"http")):
    ms = timed(lambda: col.contains(needle))
    same = np.array_equal(col.contains(needle).numpy(), masks[name].numpy())
    res["c_general_" + name] = {"pattern": "%" + needle.decode() + "%", "ms": round(ms, 4), "GBps": rate(ms), "mask_equals_flat": bool(same)}
    assert same, name
ctx.set_option("tune_str_contains_general", 0)
res["a_over_b_1pct"] = round(res["a_flat_1pct"]["GBps"] / res["b_stream_read"]["GBps"], 3)
res["a_over_b_every_row"] = round(res["a_flat_every_row"]["GBps"] / res["b_stream_read"]["GBps"], 3)
res["a_every_row_over_a_1pct"] = round(res["a_flat_every_row"]["GBps"] / res["a_flat_1pct"]["GBps"], 3)
res["a_over_c_1pct"] = round(res["a_flat_1pct"]["GBps"] / res["c_general_1pct"]["GBps"], 3)
res["a_over_c_every_row"] = round(res["a_flat_every_row"]["GBps"] / res["c_general_every_row"]["GBps"], 3)
line = json.dumps(res)
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
print(line)
