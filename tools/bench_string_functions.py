#!/usr/bin/env python3
"""The String functions on one MI355X (clickhouse_amd/csrc/string_func_kernels.hip): length, lengthUTF8, empty, lower, upper, compare_column,
substring, concat and position over HBM-resident columns, HIP-event timed on the context's stream, medians after warm-up.
Columns: the four fixed-width shapes of tools/bench_string_sort.py at `--rows` rows and the URL-like column of tools/bench_string_match.py
at `--gib` GiB of chars.  Next to every call, on the same build and in the same session: a plain device copy of that function's MODEL
BYTES -- the bytes it must read plus the bytes it must write, as a copy of half as many bytes, which reads and writes
them once -- and the ratio call / copy.  position is also timed against contains with the same needle.  Every result is checked against
plain Python `bytes` operations on the first `--sample` rows, outside the timed region.
usage: python tools/bench_string_functions.py [--rows 10000000] [--gib 1.0] [--reps 9] [--warmup 3] [--sample 4096] [--commit ID] [--out FILE]
-> one JSON line"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clickhouse_amd as ch
from clickhouse_amd.lowcardinality import ColumnString

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--gib", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sample", type=int, default=4096)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(st)
ctx = ch.Context(0, st.cuda_stream)      # torch's copies and the library's kernels share one stream, and one pair of events times both
g = torch.Generator(device=dev).manual_seed(13)
NEEDLE = b"google"


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    times = []
    for _ in range(args.reps):
        ctx.timer_start()
        out = fn()
        times.append(ctx.timer_stop_ms())
        del out
    return statistics.median(times)


def random_bytes(n, width, lo=33, hi=127):
    return torch.randint(lo, hi, (n, width), dtype=torch.int32, device=dev, generator=g).to(torch.uint8)


def city_like(n, width):
    cid = torch.randint(0, 250, (n,), dtype=torch.int64, device=dev, generator=g)
    body = torch.full((n, 10), 48, dtype=torch.uint8, device=dev)
    for k, c in enumerate(b"CITY-"):
        body[:, k] = c
    body[:, 5] = ((cid // 100) % 10 + 48).to(torch.uint8)
    body[:, 6] = ((cid // 10) % 10 + 48).to(torch.uint8)
    body[:, 9] = (cid % 10 + 48).to(torch.uint8)
    return body[:, :width].contiguous()


def url_fixed(n):
    body = torch.empty((n, 40), dtype=torch.uint8, device=dev)
    body[:, :24] = torch.tensor(list(b"https://www.example.com/"), dtype=torch.uint8, device=dev)
    body[:, 24:] = random_bytes(n, 16, 97, 123)
    return body


def wrap(offsets, chars, size):
    return ColumnString(ctx.wrap(offsets.data_ptr(), np.uint64, offsets.shape[0], keepalive=offsets), ctx.wrap(chars.data_ptr(), np.uint8, size, keepalive=chars))


def fixed_width_column(body):
    n, width = body.shape
    flat = torch.zeros(n * (width + 1) + 64, dtype=torch.uint8, device=dev)
    flat[:n * (width + 1)].view(n, width + 1)[:, :width] = body
    offs = torch.arange(1, n + 1, dtype=torch.int64, device=dev) * (width + 1)
    return wrap(offs, flat, n * (width + 1))


def url_like_column(gib):
    """tools/bench_string_match.py's column: "http://" + 32..112 bytes of [a-z./-_=0], one row in a hundred carries "google" """
    rows = int(gib * 2**30 / 80)
    lens = torch.randint(40, 121, (rows,), dtype=torch.int64, device=dev, generator=g)
    offsets = torch.cumsum(lens + 1, 0)
    size = int(offsets[-1].item())
    begins = offsets - lens - 1
    table = torch.tensor(list(b"abcdefghijklmnopqrstuvwxyz./-_=0"), dtype=torch.uint8, device=dev)
    chars = torch.empty(size + 64, dtype=torch.uint8, device=dev)
    step = 1 << 26
    for lo in range(0, size, step):
        n = min(step, size - lo)
        chars[lo:lo + n] = table[torch.randint(0, 32, (n,), dtype=torch.int64, device=dev, generator=g)]
    chars[size:] = 0
    for k, b in enumerate(b"http://"):
        chars[begins + k] = b
    planted = torch.arange(0, rows, 100, device=dev)
    for k, b in enumerate(NEEDLE):
        chars[begins[planted] + 12 + k] = b
    chars[offsets - 1] = 0
    return wrap(offsets, chars, size)


def head_values(col, k):
    """the first k values on the host"""
    k = min(k, col.size())
    if not k:
        return []
    offs = col.offsets.numpy(k)
    data = col.chars.numpy(int(offs[-1])).tobytes()
    return [data[(int(offs[i - 1]) if i else 0):int(offs[i]) - 1] for i in range(k)]


def head_numbers(column, k):
    return column.numpy(min(k, column.size())).tolist()


def copy_ms(model_bytes):
    half = max(int(model_bytes) // 2, 1)
    src = torch.empty(half, dtype=torch.uint8, device=dev)
    dst = torch.empty(half, dtype=torch.uint8, device=dev)
    ms = median_ms(lambda: dst.copy_(src))
    del src, dst
    return ms


def measure(col, name):
    rows, C = col.size(), col.chars.size()
    twin = wrap(col.offsets._keepalive.clone(), col.chars._keepalive.clone(), C)      # an equal copy at another address
    sample = head_values(col, args.sample)
    k = len(sample)
    out = {"column": name, "rows": rows, "chars_bytes": C, "mean_value_bytes": round(C / rows - 1, 2), "functions": {}}

    def record(fn_name, call, model_bytes, check, extra=None):
        check(call())
        ms = median_ms(call)
        cp = copy_ms(model_bytes)
        r = {"ms": round(ms, 4), "model_bytes": int(model_bytes), "model_GBps": round(model_bytes / ms / 1e6, 1), "copy_of_model_bytes_ms": round(cp, 4),
             "copy_GBps": round(model_bytes / cp / 1e6, 1), "call_over_copy": round(ms / cp, 2)}
        r.update(extra or {})
        out["functions"][fn_name] = r
        print(json.dumps({name: {fn_name: r}}), file=sys.stderr, flush=True)

    def numbers(want):
        return lambda res: _same(head_numbers(res, k), want)

    def strings(want):
        return lambda res: _same(head_values(res, k), want)

    record("length", col.length, 16 * rows, numbers([len(v) for v in sample]))
    record("empty", col.empty, 9 * rows, numbers([int(not v) for v in sample]))
    record("lengthUTF8", col.length_utf8, 16 * rows + C, numbers([sum(1 for b in v if (b & 0xC0) != 0x80) for v in sample]))
    record("lower", col.lower, 2 * C + 16 * rows, strings([v.lower() for v in sample]))       # bytes.lower / upper are the ASCII forms
    record("upper", col.upper, 2 * C + 16 * rows, strings([v.upper() for v in sample]))
    # a column against an equal copy of itself: no row ends early, every byte of both sides is read
    record("compare_column EQ (equal copy)", lambda: col.compare_column(ch._capi.EQ, twin), 16 * rows + 2 * C + rows, numbers([1] * k))
    sub = col.substring(2)
    record("substring(2)", lambda: col.substring(2), 16 * rows + (sub.chars.size() - rows) + sub.chars.size(), strings([v[1:] for v in sample]),
           {"result_chars_bytes": sub.chars.size()})
    del sub
    sub = col.substring(-8, 4)
    record("substring(-8, 4)", lambda: col.substring(-8, 4), 16 * rows + (sub.chars.size() - rows) + sub.chars.size(),
           strings([sub_ref(v, -8, 4) for v in sample]), {"result_chars_bytes": sub.chars.size()})
    del sub
    cat = ColumnString.concat(col, b"/", twin)
    record("concat(a, '/', b)", lambda: ColumnString.concat(col, b"/", twin), 16 * rows + 2 * C + 8 * rows + cat.chars.size(), strings([v + b"/" + v for v in sample]),
           {"result_chars_bytes": cat.chars.size()})
    del cat
    hits = int(np.count_nonzero(col.position(NEEDLE).numpy()))
    record("position('google')", lambda: col.position(NEEDLE), 16 * rows + C, numbers([v.find(NEEDLE) + 1 for v in sample]), {"rows_hit": hits})
    ms_contains = median_ms(lambda: col.contains(NEEDLE))
    assert ch.count_bytes_in_filter(col.contains(NEEDLE)) == hits
    p = out["functions"]["position('google')"]
    p["contains_same_needle_ms"] = round(ms_contains, 4)
    p["position_over_contains"] = round(p["ms"] / ms_contains, 2)
    del twin
    return out


def sub_ref(v, offset, length=None):
    """the substring window by index arithmetic (include/chgpu.h)"""
    start = offset - 1 if offset > 0 else len(v) + offset
    end = len(v) if length is None else start + length
    lo, hi = max(start, 0), min(end, len(v))
    return v[lo:hi] if hi > lo else b""


def _same(got, want):
    assert got == want, next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w)


res = {"tool": "tools/bench_string_functions.py", "commit": args.commit,
       "metric": "ms per call: median of %d calls after %d warm-up calls, HIP events on the context's stream; model bytes = bytes a function must read + write" % (args.reps, args.warmup),
       "columns": []}
shapes = [("8-byte distinct values", lambda: fixed_width_column(random_bytes(args.rows, 8))),
          ("10-byte city-like values, 250 distinct", lambda: fixed_width_column(city_like(args.rows, 10))),
          ("8-byte city-like values", lambda: fixed_width_column(city_like(args.rows, 8))),
          ("URL-like: 24-byte shared prefix + 16 random bytes", lambda: fixed_width_column(url_fixed(args.rows))),
          ("URL-like, 40..120 bytes, %.2f GiB of chars" % args.gib, lambda: url_like_column(args.gib))]
for name, make in shapes:
    col = make()
    res["columns"].append(measure(col, name))
    del col
    ctx.trim()
    torch.cuda.empty_cache()
line = json.dumps(res)
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
print(line)
