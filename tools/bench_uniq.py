#!/usr/bin/env python3
"""uniqExact(value) GROUP BY key: the UniqExact operator against the composition the library offered before it.

  new          UniqExact(UInt64, UInt64): add_block over all rows + finalize
  composition  KeyDict(16 bytes).encode((key, value)) -> key column of the ids 0..n-1 -> Aggregator count() -> finalize

Shapes, all of --rows rows of (UInt64 key, UInt64 value), rows in random order:
  a  10^3 keys x 10^3 values each        b  10^6 keys, 10^7 distinct pairs        c  every pair distinct (10^6 keys)
Each side's result is checked against numpy once (on the pair ids the rows were drawn from) before anything is timed.  Then both sides
run alternately in this one process, --rounds times after one warm-up each; a time is a host clock around work that ends in a device
synchronise.  The yardstick is the composition: `ok` says the new operator's median is no slower than the composition's median by more
than the composition's own spread (max - min over its rounds).  One JSON document on stdout, and in --out."""
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

MIX = np.uint64(0x9E3779B97F4A7C15)


def make_shape(shape, rows, rng):
    """-> (keys, values, {key: distinct count} as (sorted keys, counts))"""
    if shape == "a":
        n_keys, n_pairs = 1000, 1000 * 1000
    elif shape == "b":
        n_keys, n_pairs = 10**6, 10**7
    else:
        n_keys, n_pairs = 10**6, rows
    n_pairs = min(n_pairs, rows) if shape != "c" else rows
    n_keys = min(n_keys, n_pairs)
    pid = rng.permutation(rows).astype(np.uint64) if shape == "c" else rng.integers(0, n_pairs, size=rows, dtype=np.uint64)
    keys = pid % np.uint64(n_keys)
    values = (pid // np.uint64(n_keys)) * MIX          # distinct per (key, pid // n_keys)
    present = np.bincount(pid.astype(np.int64), minlength=n_pairs) > 0 if shape != "c" else np.ones(rows, dtype=bool)
    per_key = np.bincount(np.nonzero(present)[0] % n_keys, minlength=n_keys)
    want_keys = np.nonzero(per_key)[0].astype(np.uint64)
    return keys, values, (want_keys, per_key[per_key > 0].astype(np.uint64))


def same_result(keys, counts, want):
    o = np.argsort(keys, kind="stable")
    return np.array_equal(keys[o], want[0]) and np.array_equal(counts[o], want[1])


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
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--rounds", type=int, default=5)
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
    iota = ctx.upload(np.arange(args.rows, dtype=np.uint32))      # ids 0..n-1 for the composition, made outside the timed part

    def run_new(kcol, vcol):
        u = ch.UniqExact(np.uint64, np.uint64, ctx=ctx)
        try:
            u.add_block(kcol, vcol)
            k, c = u.finalize_columns()
            ctx.synchronize()
            return k, c
        finally:
            u.close()

    def run_composition(kcol, vcol):
        d = ch.KeyDict([np.uint64, np.uint64], ctx=ctx)
        agg = ch.Aggregator(np.uint64, [(ch.AGG_COUNT, None)], ctx=ctx)
        try:
            d.encode([kcol, vcol])
            pair_keys = d.key_columns(iota.cut(0, len(d)))[0]
            agg.execute_on_block(pair_keys, [None])
            k, (c,) = agg.finalize_columns()
            ctx.synchronize()
            return k, c
        finally:
            agg.close()
            del d

    result = {"bench": "uniq_exact", "rows": args.rows, "rounds": args.rounds, "seed": args.seed, "gpu": gpu, "shapes": {}}
    for shape in args.shapes.split(","):
        rng = np.random.Generator(np.random.PCG64(args.seed))
        keys, values, want = make_shape(shape, args.rows, rng)
        kcol, vcol = ctx.upload(keys), ctx.upload(values)
        del keys, values
        entry = {"keys": int(len(want[0])), "pairs": int(want[1].sum())}
        # correctness once, which is also the warm-up of both sides; the new side's plan line from the same run
        ctx.set_option("debug", 1)
        with captured_stderr() as box:
            k, c = run_new(kcol, vcol)
        ctx.set_option("debug", 0)
        entry["plan"] = [ln for ln in box["text"].splitlines() if "uniq plan=" in ln]
        entry["new_correct"] = bool(same_result(k.numpy(), c.numpy(), want))
        k, c = run_composition(kcol, vcol)
        entry["composition_correct"] = bool(same_result(k.numpy(), c.numpy(), want))
        del k, c
        if not (entry["new_correct"] and entry["composition_correct"]):
            entry["error"] = "a result differs from numpy: not timed"
            result["shapes"][shape] = entry
            continue
        times = {"new": [], "composition": []}
        for _ in range(args.rounds):
            for name, fn in (("new", run_new), ("composition", run_composition)):
                ctx.synchronize()
                t0 = time.perf_counter()
                out = fn(kcol, vcol)
                times[name].append((time.perf_counter() - t0) * 1e3)
                del out
        for name, ts in times.items():
            entry[name] = {"ms": [round(t, 3) for t in ts], "median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3),
                           "max_ms": round(max(ts), 3), "rows_per_s": round(args.rows / (float(np.median(ts)) * 1e-3))}
        spread = entry["composition"]["max_ms"] - entry["composition"]["min_ms"]
        entry["composition_spread_ms"] = round(spread, 3)
        entry["speedup"] = round(entry["composition"]["median_ms"] / entry["new"]["median_ms"], 3)
        entry["ok"] = bool(entry["new"]["median_ms"] <= entry["composition"]["median_ms"] + spread)
        result["shapes"][shape] = entry
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
