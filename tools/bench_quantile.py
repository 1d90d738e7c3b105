#!/usr/bin/env python3
"""quantilesExact(0.5, 0.9, 0.99)(value) GROUP BY key: the QuantileExact operator against the composition a caller could write before it.

  new          QuantileExact(UInt64, Float64): add_block over all rows + finalize
  composition  sort_permutation by value -> stably by key with the first permutation as perm_in -> index both columns ->
               Aggregator count() for the group sizes -> the ranks picked from the sorted value column (index)

Shapes, all of --rows rows of (UInt64 key, Float64 value), rows in random order:
  a  10^3 keys        b  10^6 keys        c  without key
Each side's result is checked against numpy once before anything is timed: for every group and level the answer x must be an element
with count(v < x) <= rank < count(v <= x), counted over all rows (no sort on the host).  Then both sides run alternately in this one
process, --rounds times after that first run; a time is a host clock around work that ends in a device synchronise or a download.  The
yardstick is the composition: `ok` says the new operator's median is no slower than the composition's median by more than the
composition's own spread (max - min over its rounds).  One JSON document on stdout, and in --out."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))

from quantile_exact_ref import rank  # noqa: E402  (the rank table, written once for the tests)

LEVELS = [0.5, 0.9, 0.99]
N_KEYS = {"a": 10**3, "b": 10**6, "c": 0}


def correct(group_of_row, values, n_groups, result_keys, result_cols):
    """result_keys: the group index of every result row (None: one group); result_cols: one array per level"""
    counts = np.bincount(group_of_row, minlength=n_groups) if group_of_row is not None else np.array([len(values)])
    if result_keys is None:
        result_keys = np.zeros(1, dtype=np.int64)
    if len(result_keys) != int((counts > 0).sum()) or len(np.unique(result_keys)) != len(result_keys) or (counts[result_keys] == 0).any():
        return False
    for level, col in zip(LEVELS, result_cols):
        x = np.empty(n_groups if group_of_row is not None else 1, dtype=np.float64)
        x[result_keys] = col
        per_row = x[group_of_row] if group_of_row is not None else x[0]
        if group_of_row is not None:
            lt = np.bincount(group_of_row, weights=values < per_row, minlength=n_groups)
            le = np.bincount(group_of_row, weights=values <= per_row, minlength=n_groups)
        else:
            lt, le = np.array([np.count_nonzero(values < per_row)]), np.array([np.count_nonzero(values <= per_row)])
        r = np.array([rank("exact", level, int(n)) if n else 0 for n in counts[result_keys]])
        if not ((lt[result_keys] <= r) & (r < le[result_keys])).all():
            return False
    return True


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

    def run_new(kcol, vcol):
        """-> (keys or None, [values per level]) as numpy"""
        q = ch.QuantileExact(np.uint64 if kcol is not None else None, np.float64, ctx=ctx)
        try:
            q.add_block(kcol, vcol)
            return q.finalize(LEVELS)
        finally:
            q.close()

    def run_composition(kcol, vcol):
        perm = ch.sort_permutation(vcol)
        if kcol is None:
            n = vcol.size()
            pos = ctx.upload(np.array([rank("exact", l, n) for l in LEVELS], dtype=np.uint64))
            return None, [vcol.index(perm).index(pos).numpy()[i:i + 1] for i in range(len(LEVELS))]
        perm = ch.sort_permutation(kcol, perm)
        sorted_values = vcol.index(perm)
        agg = ch.Aggregator(np.uint64, [(ch.AGG_COUNT, None)], ctx=ctx)
        try:
            agg.execute_on_block(kcol, [None])
            gk, (gc,) = agg.finalize_columns()
            gk, gc = gk.numpy(), gc.numpy()
        finally:
            agg.close()
        order = np.argsort(gk, kind="stable")                     # the sorted column holds the groups in ascending key order
        gk, gc = gk[order], gc[order].astype(np.uint64)
        starts = np.concatenate([[0], np.cumsum(gc)[:-1]]).astype(np.uint64)
        out = []
        for l in LEVELS:
            r = np.where(l < 1, (l * gc.astype(np.float64)).astype(np.uint64), gc - np.uint64(1))
            out.append(sorted_values.index(ctx.upload(starts + np.minimum(r, gc - np.uint64(1)))).numpy())
        return gk, out

    result = {"bench": "quantile_exact", "rows": args.rows, "levels": LEVELS, "rounds": args.rounds, "seed": args.seed, "gpu": gpu, "shapes": {}}
    for shape in args.shapes.split(","):
        rng = np.random.Generator(np.random.PCG64(args.seed))
        n_keys = N_KEYS[shape]
        values = rng.standard_normal(args.rows)
        keys = rng.integers(0, n_keys, size=args.rows, dtype=np.uint64) if n_keys else None
        group_of_row = keys.astype(np.int64) if keys is not None else None
        kcol, vcol = (ctx.upload(keys) if keys is not None else None), ctx.upload(values)
        entry = {"keys": n_keys}
        print(f"shape {shape}: {args.rows} rows uploaded", file=sys.stderr, flush=True)
        # correctness once, which is also the warm-up of both sides; the new side's plan lines from the same run
        ctx.set_option("debug", 1)
        with captured_stderr() as box:
            k, cols = run_new(kcol, vcol)
        ctx.set_option("debug", 0)
        entry["plan"] = [ln for ln in box["text"].splitlines() if "quantile plan=" in ln]
        entry["new_correct"] = bool(correct(group_of_row, values, n_keys, None if k is None else k.astype(np.int64), cols))
        k, cols = run_composition(kcol, vcol)
        entry["composition_correct"] = bool(correct(group_of_row, values, n_keys, None if k is None else k.astype(np.int64), cols))
        del k, cols, keys, values, group_of_row
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
                out = fn(kcol, vcol)
                times[name].append((time.perf_counter() - t0) * 1e3)
                del out
        for name, ts in times.items():
            entry[name] = {"ms": [round(t, 3) for t in ts], "median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3),
                           "max_ms": round(max(ts), 3), "rows_per_s": round(args.rows / (float(np.median(ts)) * 1e-3))}
        # where the new side's time goes: add_block, a first finalize, a finalize that reuses the groups and segments (the select alone)
        q = ch.QuantileExact(np.uint64 if kcol is not None else None, np.float64, ctx=ctx)
        ctx.synchronize()
        t0 = time.perf_counter()
        q.add_block(kcol, vcol)
        ctx.synchronize()
        t1 = time.perf_counter()
        q.finalize(LEVELS)
        t2 = time.perf_counter()
        cached = []
        for _ in range(3):
            t3 = time.perf_counter()
            q.finalize(LEVELS)
            cached.append((time.perf_counter() - t3) * 1e3)
        q.close()
        entry["phases_ms"] = {"add_block": round((t1 - t0) * 1e3, 3), "first_finalize": round((t2 - t1) * 1e3, 3), "cached_finalize": round(float(np.median(cached)), 3)}
        # the plan-level switches of the new side, each against the default in the same process (medians of --rounds runs)
        entry["ab_ms"] = {}
        for option, value in (("tune_quantile_no_lds_scatter", 1), ("tune_quantile_hist_rounds", 0)):
            ctx.set_option(option, value)
            ts = []
            for _ in range(args.rounds):
                ctx.synchronize()
                t0 = time.perf_counter()
                out = run_new(kcol, vcol)
                ts.append((time.perf_counter() - t0) * 1e3)
                del out
            ctx.set_option(option, 4 if option == "tune_quantile_hist_rounds" else 0)
            entry["ab_ms"][f"{option}={value}"] = round(float(np.median(ts)), 3)
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
