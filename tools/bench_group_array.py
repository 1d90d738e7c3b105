#!/usr/bin/env python3
"""groupArray(value) GROUP BY key: the GroupArray operator against the composition a caller could write before it.

  new          GroupArray(UInt64, Float64[, N]): add_block over all rows + finalize, keys and offsets downloaded
  composition  sort_permutation(keys) (stable, sizeof(key) radix passes) -> index(values, perm) -> Aggregator count() for the array
               lengths -> the group keys ordered ON THE DEVICE (sort_permutation + index of the keys and counts), then downloaded; the
               offsets are a cumsum of the counts on the host; groupArray(10) then picks the first 10 places of every group (index);
               without key the composition is a device copy of the value column (concat of one column).  Its parts are also timed
               alone in every round: `parts_ms` gives the medians of sort + index, of the count() GROUP BY with its ordering and
               download, and of the host work (cumsum, the positions of groupArray(10)).

Shapes, all of --rows rows of (UInt64 key, Float64 value), rows in random order:
  a  10^3 keys      b  10^6 keys      c  without key      d  10^6 distinct hash-like keys, all 8 bytes vary      e  groupArray(10), 10^3 keys
Each side's result is checked against numpy once before anything is timed (a stable argsort of the keys; the arrays bit for bit).  Then
both sides run alternately in this one process, --rounds times after that first run; a time is a host clock around work that ends in a
download.  The yardstick is the composition: `ok` says the new operator's median is no slower than the composition's median by more than
the composition's own spread (max - min over its rounds).  Both sides make their operator anew in every round (the new side's store
starts empty and grows in one step); `phases_ms` also gives one operator fed the same rows in --blocks blocks, where the doubling store
copies itself as it grows.  One JSON document on stdout, and in --out."""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"a": dict(keys=10**3), "b": dict(keys=10**6), "c": dict(keys=0), "d": dict(keys=10**6, hashed=True), "e": dict(keys=10**3, max_size=10)}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


@contextlib.contextmanager
def captured_stderr():
    """the library's `debug` lines are written by C code: catch file descriptor 2"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        box = {}
        try:
            yield box
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            box["text"] = f.read().decode("utf-8", "replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--shapes", default="a,b,c,d,e")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import clickhouse_amd as ch
    try:
        import torch
        gpu = {"name": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")}
    except Exception as e:  # the numbers still stand without the name
        gpu = {"name": "unknown", "error": repr(e)}
    ctx = ch.Context(0)

    def run_new(kcol, vcol, max_size, download_data=False):
        """-> (keys or None, offsets, data Column or ndarray)"""
        g = ch.GroupArray(np.uint64 if kcol is not None else None, np.float64, max_size=max_size, ctx=ctx)
        try:
            g.add_block(kcol, vcol)
            k, off, data = g.finalize_columns()
            return (k.numpy() if k is not None else None), off.numpy(), (data.numpy() if download_data else data)
        finally:
            g.close()

    parts = {"sort_index": [], "count_groups": [], "host": []}

    def run_composition(kcol, vcol, max_size, download_data=False):
        if kcol is None:
            data = ch.concat([vcol])
            off = np.array([vcol.size()], dtype=np.uint64)
            return None, off, (data.numpy() if download_data else data)
        t0 = time.perf_counter()
        perm = ch.sort_permutation(kcol)
        data = vcol.index(perm)
        ctx.synchronize()
        t1 = time.perf_counter()
        agg = ch.Aggregator(np.uint64, [(ch.AGG_COUNT, None)], ctx=ctx)
        try:
            agg.execute_on_block(kcol, [None])
            gk, (gc,) = agg.finalize_columns()
            order = ch.sort_permutation(gk)                       # the sorted column holds the groups in ascending key order
            gk, gc = gk.index(order).numpy(), gc.index(order).numpy()
        finally:
            agg.close()
        t2 = time.perf_counter()
        gc = gc.astype(np.int64)
        gather = 0.0
        if max_size:
            starts = np.cumsum(gc) - gc
            kept = np.minimum(gc, max_size)
            first = np.cumsum(kept) - kept
            pos = (np.repeat(starts, kept) + (np.arange(int(kept.sum())) - np.repeat(first, kept))).astype(np.uint64)
            t3 = time.perf_counter()
            data = data.index(ctx.upload(pos))
            ctx.synchronize()
            gather = time.perf_counter() - t3                     # device work: counted with sort + index, not with the host's
            gc = kept
        off = np.cumsum(gc).astype(np.uint64)
        t4 = time.perf_counter()
        parts["sort_index"].append((t1 - t0 + gather) * 1e3)
        parts["count_groups"].append((t2 - t1) * 1e3)
        parts["host"].append((t4 - t2 - gather) * 1e3)
        return gk, off, (data.numpy() if download_data else data)

    def correct(got, want):
        gk, off, data = got
        wk, woff, wdata = want
        if wk is None:
            return gk is None and np.array_equal(off, woff) and same_bits(data, wdata)
        return gk is not None and np.array_equal(gk, wk) and np.array_equal(off, woff) and same_bits(data, wdata)   # (both sides: ascending keys)

    result = {"bench": "group_array", "rows": args.rows, "rounds": args.rounds, "seed": args.seed, "gpu": gpu, "shapes": {}}
    for shape in args.shapes.split(","):
        spec = SHAPES[shape]
        rng = np.random.Generator(np.random.PCG64(args.seed))
        n_keys, max_size = spec["keys"], spec.get("max_size", 0)
        values = rng.standard_normal(args.rows)
        keys = None
        if n_keys:
            ids = rng.integers(0, n_keys, size=args.rows, dtype=np.int64)
            if spec.get("hashed"):
                pool = np.unique(rng.integers(0, 2**64 - 1, size=n_keys, dtype=np.uint64, endpoint=True))
                keys = pool[ids % len(pool)]
            else:
                keys = ids.astype(np.uint64)
            del ids
        # the numpy reference: a stable argsort of the keys, a split, max_size
        if keys is None:
            want = (None, np.array([args.rows], dtype=np.uint64), values)
        else:
            order = np.argsort(keys, kind="stable")
            sk = keys[order]
            heads = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
            counts = np.diff(np.concatenate([heads, [len(sk)]]))
            data = values[order]
            if max_size:
                kept = np.minimum(counts, max_size)
                data = data[(np.arange(len(sk)) - np.repeat(heads, counts)) < np.repeat(kept, counts)]
                counts = kept
            want = (sk[heads], np.cumsum(counts).astype(np.uint64), data)
            del order, sk, heads, counts
        kcol, vcol = (ctx.upload(keys) if keys is not None else None), ctx.upload(values)
        entry = {"keys": n_keys, "max_size": max_size, "hashed": bool(spec.get("hashed"))}
        print(f"shape {shape}: {args.rows} rows uploaded", file=sys.stderr, flush=True)
        # correctness once, which is also the warm-up of both sides; the new side's plan lines from the same run
        ctx.set_option("debug", 1)
        with captured_stderr() as box:
            got = run_new(kcol, vcol, max_size, download_data=True)
        ctx.set_option("debug", 0)
        entry["plan"] = [ln for ln in box["text"].splitlines() if "group_array plan=" in ln]
        entry["new_correct"] = bool(correct(got, want))
        got = run_composition(kcol, vcol, max_size, download_data=True)
        entry["composition_correct"] = bool(correct(got, want))
        del got, want, keys, values
        print(f"shape {shape}: new_correct={entry['new_correct']} composition_correct={entry['composition_correct']}", file=sys.stderr, flush=True)
        if not (entry["new_correct"] and entry["composition_correct"]):
            entry["error"] = "a result differs from numpy: not timed"
            result["shapes"][shape] = entry
            continue
        times = {"new": [], "composition": []}
        for _ in range(args.rounds):
            for name, fn in (("new", run_new), ("composition", run_composition)):
                ctx.synchronize()
                t0 = time.perf_counter()
                out = fn(kcol, vcol, max_size)
                ctx.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
                del out
        if kcol is not None:
            entry["composition_parts_ms"] = {k: round(float(np.median(v[-args.rounds:])), 3) for k, v in parts.items()}
        for name, ts in times.items():
            entry[name] = {"ms": [round(t, 3) for t in ts], "median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3),
                           "max_ms": round(max(ts), 3), "rows_per_s": round(args.rows / (float(np.median(ts)) * 1e-3))}
        # where the new side's time goes: add_block, a first finalize, a finalize that reuses the segments
        g = ch.GroupArray(np.uint64 if kcol is not None else None, np.float64, max_size=max_size, ctx=ctx)
        ctx.synchronize()
        t0 = time.perf_counter()
        g.add_block(kcol, vcol)
        ctx.synchronize()
        t1 = time.perf_counter()
        out = g.finalize_columns()
        ctx.synchronize()
        t2 = time.perf_counter()
        del out
        out = g.finalize_columns()
        ctx.synchronize()
        t3 = time.perf_counter()
        del out
        g.close()
        entry["phases_ms"] = {"add_block": round((t1 - t0) * 1e3, 3), "first_finalize": round((t2 - t1) * 1e3, 3), "cached_finalize": round((t3 - t2) * 1e3, 3)}
        # the same rows in --blocks blocks into one operator: the doubling store copies what it holds every time it grows
        g = ch.GroupArray(np.uint64 if kcol is not None else None, np.float64, max_size=max_size, ctx=ctx)
        step = (args.rows + args.blocks - 1) // args.blocks
        ctx.synchronize()
        t0 = time.perf_counter()
        for b in range(0, args.rows, step):
            g.add_block(kcol, vcol, row_begin=b, row_end=min(args.rows, b + step))
        ctx.synchronize()
        t1 = time.perf_counter()
        g.close()
        entry["phases_ms"][f"add_in_{args.blocks}_blocks"] = round((t1 - t0) * 1e3, 3)
        spread = entry["composition"]["max_ms"] - entry["composition"]["min_ms"]
        entry["composition_spread_ms"] = round(spread, 3)
        entry["speedup"] = round(entry["composition"]["median_ms"] / entry["new"]["median_ms"], 3)
        entry["ok"] = bool(entry["new"]["median_ms"] <= entry["composition"]["median_ms"] + spread)
        result["shapes"][shape] = entry
        print(f"shape {shape}: new {entry['new']['median_ms']} ms, composition {entry['composition']['median_ms']} ms", file=sys.stderr, flush=True)
        del kcol, vcol
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
