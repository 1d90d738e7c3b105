#!/usr/bin/env python3
"""Window frames of chgpu_window_evaluate_framed: min / max over frames bounded on both sides and RANGE frames with offsets, each beside
today's one-sided max and ROWS sum and beside a column copy, all measured in the same run (the method of tools/bench_window.py).

Input: --rows rows of (UInt32 partition key, Int64 order key, Int64 value), already sorted by (key, order), at 10^3, 10^6 and --rows
partitions of equal length; the order key pairs rows up (t = i // 2), so every second row is a peer head and an offset of k reaches
about 2 k rows.

Timed with HIP events on the context's stream (no download inside a time), one warm-up round, then --rounds rounds; a figure is the
median with min and max beside it.  Every round makes a NEW handle and calls, in this order:
  one_sided_max   max over ROWS UNBOUNDED PRECEDING .. UNBOUNDED FOLLOWING   (Window.max: the running extremum, as before)
  rows_sum        sum over ROWS 9 PRECEDING .. CURRENT ROW                   (Window.sum: the prefix sums, as before)
  max_rows_9      max over ROWS 9 PRECEDING .. CURRENT ROW                   (block masks; a frame mostly inside one block)
  max_rows_1000   max over ROWS 1000 PRECEDING .. 1000 FOLLOWING             (block masks + sparse table, 5 levels)
  sum_range_10    sum over RANGE 10 PRECEDING .. CURRENT ROW                 (one searched bound + the prefix sums)
  max_range_10    max over RANGE 10 PRECEDING .. CURRENT ROW                 (one searched bound + masks + every level of the table)
  sum_range_1e6   sum over RANGE 10^6 PRECEDING .. 10^6 FOLLOWING            (two searched bounds that gallop to the partition's edges)
so a call's `first` time includes the bound arrays it is the first to need; the same calls are then repeated on the warm handle
(`warm`: bounds cached -- the searched fs / fe, the masks and the table are a call's temporaries and are built by every call).

Yardstick: chgpu_col_concat of one column is a copy, 2 x its bytes; the best rate over the three columns is this build's streaming rate.
A call's `bytes_per_row` is what its kernels move by their design (the gallop's loads beyond the row's own come from
cache and are not counted); `fraction_of_streaming` is the time those bytes take at that rate over the warm time.  `slower` marks a new
call whose warm time exceeds that of the old call of its kind (one_sided_max, rows_sum) by more than its extra bytes at the streaming
rate explain.
Also the numpy reference (tests/window_frames_ref.py, fast form) on one core over the first --ref-rows rows, as ns per row.
The device results are checked against it over the first --check-rows rows (whole partitions) before anything is timed.  One JSON
document on stdout, and in --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

# bytes per row of the warm call, by the kernels' design: streamed reads + gathers + writes
SEARCH = 8 + 4 + 4                                  # one searched bound: x[i], ps or pe, the u32 written
MASKS = 8 + 8                                       # the block masks: x in, a u64 mask out (the table's levels: 8 B per 64 rows each)
BYTES = {
    "one_sided_max": (8 + 4) + (8 + 4 + 8) + (4 + 4 + 8 + 8),
    "rows_sum": 8 + (8 + 8) + (4 + 16 + 8),
    "max_rows_9": MASKS + (4 + 8 + 8 + 8),          # ps, mask[last], x[at], result
    "max_rows_1000": MASKS + (4 + 4 + 16 + 16 + 16 + 8),  # ps, pe, two masks, two values, two cells of the table, result
    "sum_range_10": SEARCH + 8 + (8 + 8) + (4 + 4 + 4 + 16 + 8),  # + tile sums; prefix apply; ps, ge, fs, P[fe], P[fs], result
    "max_range_10": SEARCH + MASKS + (4 + 4 + 4 + 8 + 8 + 8),
    "sum_range_1e6": 2 * SEARCH + 8 + (8 + 8) + (4 + 4 + 4 + 4 + 16 + 8),
}
OLD_OF = {"max_rows_9": "one_sided_max", "max_rows_1000": "one_sided_max", "max_range_10": "one_sided_max", "sum_range_10": "rows_sum",
          "sum_range_1e6": "rows_sum"}


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--partitions", default="1000,1000000,rows")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ref-rows", type=int, default=10_000_000)
    ap.add_argument("--check-rows", type=int, default=200_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import clickhouse_amd as ch
    import window_frames_ref as F
    import window_ref as R
    try:
        import torch
        gpu = {"name": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")}
    except Exception as e:  # the numbers still stand without the name
        gpu = {"name": "unknown", "error": repr(e)}
    ctx = ch.Context(0)
    K = ch._capi
    rows = args.rows
    whole = ch.Frame.rows(ch.UNBOUNDED, ch.UNBOUNDED)
    frames = {"one_sided_max": (R.ROWS, R.UNBOUNDED_PRECEDING, 0, R.UNBOUNDED_FOLLOWING, 0),
              "rows_sum": (R.ROWS, R.OFFSET_PRECEDING, 9, R.CURRENT_ROW, 0),
              "max_rows_9": (R.ROWS, R.OFFSET_PRECEDING, 9, R.CURRENT_ROW, 0),
              "max_rows_1000": (R.ROWS, R.OFFSET_PRECEDING, 1000, R.OFFSET_FOLLOWING, 1000),
              "sum_range_10": (R.RANGE, R.OFFSET_PRECEDING, 10, R.CURRENT_ROW, 0),
              "max_range_10": (R.RANGE, R.OFFSET_PRECEDING, 10, R.CURRENT_ROW, 0),
              "sum_range_1e6": (R.RANGE, R.OFFSET_PRECEDING, 10**6, R.OFFSET_FOLLOWING, 10**6)}
    function_of = {name: (R.MAX if "max" in name else R.SUM) for name in frames}

    def frame_of(f):
        def bound(kind, off):
            return ch.CURRENT_ROW if kind == R.CURRENT_ROW else ch.preceding(off) if kind == R.OFFSET_PRECEDING else ch.following(off)
        return ch.Frame(f[0], bound(f[1], f[2]), bound(f[3], f[4]))

    def timed(fn):
        ctx.timer_start()
        out = fn()
        return ctx.timer_stop_ms(), out

    def calls(w, tcol, xcol):
        out = [("one_sided_max", lambda: w.evaluate_column(K.WIN_MAX, whole, xcol)),
               ("rows_sum", lambda: w.evaluate_column(K.WIN_SUM, frame_of(frames["rows_sum"]), xcol))]
        for name in ("max_rows_9", "max_rows_1000", "sum_range_10", "max_range_10", "sum_range_1e6"):
            fw = w.over(frame_of(frames[name]), order=tcol if F.has_range_offset(frames[name]) else None)
            out.append((name, lambda fw=fw, name=name: fw.evaluate_column(function_of[name], xcol)))
        return out

    result = {"bench": "window_frames", "rows": rows, "rounds": args.rounds, "seed": args.seed, "gpu": gpu, "bytes_per_row": BYTES, "shapes": {}}
    for spec in args.partitions.split(","):
        n_part = rows if spec == "rows" else min(int(spec), rows)
        rng = np.random.Generator(np.random.PCG64(args.seed))
        idx = np.arange(rows, dtype=np.int64)
        p = (idx * n_part // rows).astype(np.uint32)
        t = idx // 2
        x = rng.integers(-2**40, 2**40, size=rows, dtype=np.int64)
        del idx
        pcol, tcol, xcol = ctx.upload(p), ctx.upload(t), ctx.upload(x)
        entry = {"partitions": n_part}
        print(f"partitions {n_part}: {rows} rows uploaded", file=sys.stderr, flush=True)

        if not args.no_check:
            # frames never leave a partition: a prefix of whole partitions has the results of the whole input
            m = min(rows, 4 * args.check_rows + 1)
            heads = np.flatnonzero(R.heads_fast([p[:m]], [], m)[0])
            ends = heads[heads >= min(args.check_rows, rows)]
            n = int(ends[0]) if len(ends) else rows if m == rows else int(heads[-1]) if heads[-1] else m
            w = ch.Window([pcol], [tcol], ctx=ctx)
            ok = True
            for name, fn in calls(w, tcol, xcol):
                col = fn()
                got = col.numpy()[:n]
                col.free()
                ok = ok and R.same_bits(got, F.window_fast(function_of[name], [p[:n]], [t[:n]], n, frames[name], x[:n]))
            w.close()
            entry["correct"], entry["checked_rows"] = bool(ok), n
            print(f"partitions {n_part}: correct={ok} over the first {n} rows", file=sys.stderr, flush=True)
            if not ok:
                entry["error"] = "a result differs from the reference: not timed"
                result["shapes"][str(n_part)] = entry
                continue

        first, warm = {}, {}
        for rnd in range(args.rounds + 1):
            w = ch.Window([pcol], [tcol], ctx=ctx)
            for into in (first, warm):
                for name, fn in calls(w, tcol, xcol):
                    ms, out = timed(fn)
                    out.free()
                    if rnd:                                          # round 0 is the warm-up: first use of every kernel, the pool's first allocations
                        into.setdefault(name, []).append(ms)
            w.close()

        copies = {}
        for name, col, width in (("key_u32", pcol, 4), ("order_i64", tcol, 8), ("value_i64", xcol, 8)):
            ts = []
            for rnd in range(args.rounds + 1):
                ms, out = timed(lambda: ch.concat([col]))
                out.free()
                if rnd:
                    ts.append(ms)
            copies[name] = dict(stats(ts), gb_per_s=round(2 * width * rows / (float(np.median(ts)) * 1e-3) / 1e9, 1))
        rate = max(c["gb_per_s"] for c in copies.values()) * 1e9
        entry["copy"] = copies
        entry["streaming_gb_per_s"] = round(rate / 1e9, 1)

        entry["calls"] = {}
        for name in first:
            e = {"first": stats(first[name]), "warm": stats(warm[name]), "bytes_per_row": BYTES[name]}
            ms = e["warm"]["median_ms"]
            e["fraction_of_streaming"] = round(BYTES[name] * rows / rate * 1e3 / ms, 3) if ms > 0 else None
            entry["calls"][name] = e
        for name, old in OLD_OF.items():
            e, o = entry["calls"][name], entry["calls"][old]
            extra_ms = max(0, BYTES[name] - BYTES[old]) * rows / rate * 1e3
            e["vs_" + old] = round(e["warm"]["median_ms"] / o["warm"]["median_ms"], 3) if o["warm"]["median_ms"] > 0 else None
            e["slower"] = bool(e["warm"]["median_ms"] > o["warm"]["median_ms"] + extra_ms)
        print(f"partitions {n_part}: " + ", ".join(f"{k} {v['warm']['median_ms']}" for k, v in entry["calls"].items())
              + f" ms; streaming {entry['streaming_gb_per_s']} GB/s", file=sys.stderr, flush=True)

        n = min(args.ref_rows, rows)
        ref = {}
        for name in frames:
            t0 = time.perf_counter()
            F.window_fast(function_of[name], [p[:n]], [t[:n]], n, frames[name], x[:n])
            ref[name] = round((time.perf_counter() - t0) / n * 1e9, 2)
        entry["numpy_one_core_ns_per_row"] = dict(ref, rows=n)
        result["shapes"][str(n_part)] = entry
        del pcol, tcol, xcol, p, t, x
        ctx.trim()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
