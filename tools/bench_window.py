#!/usr/bin/env python3
"""Window functions over a sorted block: the Window operator's calls, each against two yardsticks measured in the same run.

Input: --rows rows of (UInt32 partition key, Int64 order key, Int64 value), already sorted by (key, order), at 10^3, 10^6 and --rows
partitions of equal length; the order key pairs rows up, so every second row is a peer head.

Timed with HIP events on the context's stream (no download inside a time), one warm-up round, then --rounds rounds; a figure is the
median with min and max beside it.  Every round makes a NEW handle and calls, in this order:
  create, row_number, rank, running sum (ROWS UNBOUNDED PRECEDING .. CURRENT ROW), sliding sum (ROWS 9 PRECEDING .. CURRENT ROW),
  partition max (ROWS UNBOUNDED PRECEDING .. UNBOUNDED FOLLOWING), lagInFrame(x, 1) over the whole partition
so a call's `first` time includes the bound arrays it is the first to need (row_number builds ps, rank gs, max pe); the same calls are
then repeated on the warm handle (`warm`: bounds cached).

Yardsticks:
  (a) streaming: chgpu_col_concat of one column is a copy, 2 x its bytes; the best rate over the three columns is this build's streaming
      rate.  A call's `bytes_per_row` is what its kernels move by their design; `fraction_of_streaming` is the time those
      bytes take at that rate over the warm time.
  (b) the device sort the window follows: sort_permutation(order) -> sort_permutation(key, perm) -> index of the three columns, over the
      same rows shuffled; `vs_sort` is a call's warm time over it.
Also the vectorised numpy reference (tests/window_ref.py) on one core over the first --ref-rows rows, as ns per row.
The device results are checked against numpy once per shape before anything is timed.  One JSON document on stdout, and in --out."""
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
BYTES = {
    "create": 4 + 8 + 1,                       # the two key columns once (the neighbour row comes from cache), one flag byte
    "bound": 1 + 4,                            # one lazily built array: flags in, u32 out
    "row_number": 4 + 8,                       # ps, result
    "rank": 4 + 4 + 8,                         # ps, gs, result
    "running_sum": 8 + (8 + 8) + (4 + 16 + 8),  # tile sums; prefix apply; ps + P[fe], P[fs] + result
    "sliding_sum": 8 + (8 + 8) + (4 + 16 + 8),
    "partition_max": (8 + 4) + (8 + 4 + 8) + (4 + 4 + 8 + 8),  # tile aggregates; running max; ps, pe, M[fe - 1], result
    "lag": 4 + 4 + 8 + 8,                      # ps, pe, x[i - 1], result
}


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--partitions", default="1000,1000000,rows")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ref-rows", type=int, default=10_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import clickhouse_amd as ch
    import window_ref as R
    try:
        import torch
        gpu = {"name": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")}
    except Exception as e:  # the numbers still stand without the name
        gpu = {"name": "unknown", "error": repr(e)}
    ctx = ch.Context(0)
    rows = args.rows
    running = ch.Frame.rows(ch.UNBOUNDED, ch.CURRENT_ROW)
    sliding = ch.Frame.rows(ch.preceding(9), ch.CURRENT_ROW)
    whole = ch.Frame.rows(ch.UNBOUNDED, ch.UNBOUNDED)
    K = ch._capi
    R_RUNNING = (R.ROWS, R.UNBOUNDED_PRECEDING, 0, R.CURRENT_ROW, 0)
    R_SLIDING = (R.ROWS, R.OFFSET_PRECEDING, 9, R.CURRENT_ROW, 0)
    R_WHOLE = (R.ROWS, R.UNBOUNDED_PRECEDING, 0, R.UNBOUNDED_FOLLOWING, 0)

    def timed(fn):
        ctx.timer_start()
        out = fn()
        return ctx.timer_stop_ms(), out

    def calls(w, xcol):
        return [("row_number", lambda: w.evaluate_column(K.WIN_ROW_NUMBER)),
                ("rank", lambda: w.evaluate_column(K.WIN_RANK)),
                ("running_sum", lambda: w.evaluate_column(K.WIN_SUM, running, xcol)),
                ("sliding_sum", lambda: w.evaluate_column(K.WIN_SUM, sliding, xcol)),
                ("partition_max", lambda: w.evaluate_column(K.WIN_MAX, whole, xcol)),
                ("lag", lambda: w.evaluate_column(K.WIN_LAG_IN_FRAME, whole, xcol, 1, 0))]

    result = {"bench": "window", "rows": rows, "rounds": args.rounds, "seed": args.seed, "gpu": gpu, "bytes_per_row": BYTES, "shapes": {}}
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
            w = ch.Window([pcol], [tcol], ctx=ctx)
            part, peer = R.heads_fast([p], [t], rows)
            ok = w.counts() == (rows, int(part.sum()), int(peer.sum()))
            ok = ok and R.same_bits(w.row_number(), R.window_fast(R.ROW_NUMBER, [p], [t], rows))
            ok = ok and R.same_bits(w.rank(), R.window_fast(R.RANK, [p], [t], rows))
            ok = ok and R.same_bits(w.sum(xcol, running), R.window_fast(R.SUM, [p], [t], rows, R_RUNNING, x))
            ok = ok and R.same_bits(w.sum(xcol, sliding), R.window_fast(R.SUM, [p], [t], rows, R_SLIDING, x))
            starts = np.flatnonzero(part)
            want_max = np.repeat(np.maximum.reduceat(x, starts), np.diff(np.append(starts, rows)))
            ok = ok and R.same_bits(w.max(xcol, whole), want_max)
            ok = ok and R.same_bits(w.lag_in_frame(xcol, 1, 0, whole), R.window_fast(R.LAG_IN_FRAME, [p], [t], rows, R_WHOLE, x, offset=1, default=np.int64(0)))
            w.close()
            del part, peer, starts, want_max
            entry["correct"] = bool(ok)
            print(f"partitions {n_part}: correct={ok}", file=sys.stderr, flush=True)
            if not ok:
                entry["error"] = "a result differs from numpy: not timed"
                result["shapes"][str(n_part)] = entry
                continue

        first = {"create": []}
        warm = {}
        for rnd in range(args.rounds + 1):
            ms, w = timed(lambda: ch.Window([pcol], [tcol], ctx=ctx))
            row = {"create": ms}
            for name, fn in calls(w, xcol):
                ms, out = timed(fn)
                out.free()
                row[name] = ms
            again = {}
            for name, fn in calls(w, xcol):
                ms, out = timed(fn)
                out.free()
                again[name] = ms
            w.close()
            if rnd == 0:
                continue   # warm-up: first use of every kernel, the pool's first allocations
            for k, v in row.items():
                first.setdefault(k, []).append(v)
            for k, v in again.items():
                warm.setdefault(k, []).append(v)

        # (a) streaming rate: a copy of each column
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

        # (b) the sort the window follows, over the same rows shuffled
        shuffle = rng.permutation(rows)
        sp, st, sx = ctx.upload(p[shuffle]), ctx.upload(t[shuffle]), ctx.upload(x[shuffle])
        del shuffle
        ts = []
        for rnd in range(args.rounds + 1):
            def sort():
                perm = ch.sort_permutation(sp, ch.sort_permutation(st))
                return [c.index(perm) for c in (sp, st, sx)]
            ms, outs = timed(sort)
            for c in outs:
                c.free()
            if rnd:
                ts.append(ms)
        entry["sort"] = stats(ts)
        sort_ms = entry["sort"]["median_ms"]
        for c in (sp, st, sx):
            c.free()

        entry["calls"] = {}
        for name in first:
            e = {"first": stats(first[name])}
            if name in warm:
                e["warm"] = stats(warm[name])
            ms = e.get("warm", e["first"])["median_ms"]
            e["bytes_per_row"] = BYTES[name]
            e["fraction_of_streaming"] = round(BYTES[name] * rows / rate * 1e3 / ms, 3) if ms > 0 else None
            e["vs_sort"] = round(ms / sort_ms, 4) if sort_ms > 0 else None
            entry["calls"][name] = e
        print(f"partitions {n_part}: " + ", ".join(f"{k} {v.get('warm', v['first'])['median_ms']}" for k, v in entry["calls"].items())
              + f" ms; sort {sort_ms} ms; streaming {entry['streaming_gb_per_s']} GB/s", file=sys.stderr, flush=True)

        # the vectorised numpy reference on one core, over a prefix
        n = min(args.ref_rows, rows)
        pr, tr, xr = p[:n], t[:n], x[:n]
        ref = {}
        for name, fn in (("row_number", lambda: R.window_fast(R.ROW_NUMBER, [pr], [tr], n)),
                         ("rank", lambda: R.window_fast(R.RANK, [pr], [tr], n)),
                         ("running_sum", lambda: R.window_fast(R.SUM, [pr], [tr], n, R_RUNNING, xr)),
                         ("sliding_sum", lambda: R.window_fast(R.SUM, [pr], [tr], n, R_SLIDING, xr)),
                         ("partition_max", lambda: R.window_fast(R.MAX, [pr], [tr], n, R_WHOLE, xr)),
                         ("lag", lambda: R.window_fast(R.LAG_IN_FRAME, [pr], [tr], n, R_WHOLE, xr, offset=1, default=np.int64(0)))):
            t0 = time.perf_counter()
            fn()
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
