#!/usr/bin/env python3
"""SELECT DISTINCT key / LIMIT 5 BY key over one UInt64 column: the LimitBy operator against the composition a caller could write
before it.

  new          LimitBy(UInt64, length): filter_block over all rows -> the UInt8 filter (resident in HBM) and the number of survivors
  composition  sort_permutation(keys) (stable) -> index(keys, perm) -> Window(partition_by=sorted keys).row_number -> cmp_const(<= length)
               -> filter(perm) = the survivors' row numbers -> sort_permutation + index of those: the survivors' rows in row order
               (resident in HBM).  One block only: nothing is carried to a next one.

Shapes, all of --rows UInt64 keys in random order: a 10^3 keys, b 10^6 keys, c every key distinct, d all rows one key; each for DISTINCT
(length 1) and LIMIT 5 BY.  Checks before anything is timed: at --check-rows rows (same generator) both sides against numpy (stable
argsort, rank within run); at full size the two sides against each other (flatnonzero of the filter == the composition's rows) and the
survivor count against numpy's count of distinct keys.  Then both sides run alternately in this one process, --rounds times after that
first run; a time is a host clock around synchronised work.  `ok` says the operator's median is no slower than the composition's median
by more than the composition's own spread (max - min over its rounds).  The operator is made anew in every round, without a size hint
(`new`) and with the number of keys as hint (`new_hinted`, reported beside it, not part of `ok`).  `streamed`: one operator fed the same rows in --block-rows
blocks -- no yardstick exists for that form; rows/s and bytes/s against the plan's algorithmic bytes.  One JSON document on stdout,
and in --out."""
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

SHAPES = {"a": 10**3, "b": 10**6, "c": 0, "d": 1}   # number of keys; 0: every key distinct
CLAUSES = {"distinct": 1, "limit5": 5}
# algorithmic bytes per row of a block of 8-byte keys whose rows all take the plan: dead = key + slot + filter byte
PLAN_BYTES = {"dead": 8 + 4 + 1, "claim": 8 + 4 + 1 + 4 + 8 + 8 + 8 + 8 + 1, "rank": None}


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


def make_keys(rng, rows, n_keys):
    if n_keys == 0:
        return rng.permutation(rows).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    if n_keys == 1:
        return np.full(rows, 0xC0FFEE, dtype=np.uint64)
    return rng.integers(0, n_keys, size=rows, dtype=np.int64).astype(np.uint64)


def numpy_rows(keys, length):
    """the survivors' rows, ascending"""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    head = np.concatenate(([True], sk[1:] != sk[:-1]))
    starts = np.flatnonzero(head)
    rank = np.arange(sk.shape[0]) - starts[np.cumsum(head) - 1]
    return np.sort(order[rank < length]).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--check-rows", type=int, default=1_000_000)
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--clauses", default="distinct,limit5")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-rows", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import clickhouse_amd as ch
    from clickhouse_amd import _capi as K
    try:
        import torch
        gpu = {"name": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")}
    except Exception as e:  # the numbers still stand without the name
        gpu = {"name": "unknown", "error": repr(e)}
    ctx = ch.Context(0)

    def run_new(kcol, length, hint=0):
        op = ch.LimitBy(np.uint64, length, size_hint=hint, ctx=ctx)
        try:
            return op.filter_block(kcol)
        finally:
            op.close()

    def run_composition(kcol, length):
        perm = ch.sort_permutation(kcol)
        sk = kcol.index(perm)
        w = ch.Window(partition_by=[sk], ctx=ctx)
        try:
            rn = w.evaluate_column(K.WIN_ROW_NUMBER)
        finally:
            w.close()
        mask = ch.cmp_const(rn, ch.LE, length)
        rows = perm.filter(mask)
        return rows.index(ch.sort_permutation(rows))

    result = {"bench": "limit_by", "rows": args.rows, "check_rows": args.check_rows, "rounds": args.rounds, "block_rows": args.block_rows, "seed": args.seed,
              "gpu": gpu, "shapes": {}}
    for shape in args.shapes.split(","):
        n_keys = SHAPES[shape]
        # both sides against numpy at the small size
        small = make_keys(np.random.Generator(np.random.PCG64(args.seed)), args.check_rows, n_keys)
        scol = ctx.upload(small)
        small_ok = {}
        for clause in args.clauses.split(","):
            want = numpy_rows(small, CLAUSES[clause])
            filt, passed = run_new(scol, CLAUSES[clause])
            new_ok = passed == want.shape[0] and np.array_equal(np.flatnonzero(filt.numpy()).astype(np.uint64), want)
            comp_ok = np.array_equal(run_composition(scol, CLAUSES[clause]).numpy().astype(np.uint64), want)
            small_ok[clause] = (bool(new_ok), bool(comp_ok))
        del scol, small
        keys = make_keys(np.random.Generator(np.random.PCG64(args.seed)), args.rows, n_keys)
        distinct_keys = args.rows if n_keys == 0 else n_keys   # (at >= 100 rows a key every key of the domain is drawn)
        kcol = ctx.upload(keys)
        del keys
        print(f"shape {shape}: {args.rows} rows uploaded, {distinct_keys} keys", file=sys.stderr, flush=True)
        for clause in args.clauses.split(","):
            length = CLAUSES[clause]
            entry = {"keys": distinct_keys, "length": length, "new_correct_small": small_ok[clause][0], "composition_correct_small": small_ok[clause][1]}
            # full size, which is also the warm-up of both sides: the two sides against each other; the operator's plan line from this run
            ctx.set_option("debug", 1)
            with captured_stderr() as box:
                filt, passed = run_new(kcol, length)
            ctx.set_option("debug", 0)
            entry["plan"] = [ln for ln in box["text"].splitlines() if "limit_by plan=" in ln]
            rows = run_composition(kcol, length).numpy()
            entry["sides_agree"] = bool(passed == rows.shape[0] and np.array_equal(np.flatnonzero(filt.numpy()), rows.astype(np.int64)))
            entry["passed"] = passed
            entry["passed_plausible"] = bool(passed >= distinct_keys and passed <= distinct_keys * length)
            del filt, rows
            name = f"{shape}_{clause}"
            if not (all(small_ok[clause]) and entry["sides_agree"] and entry["passed_plausible"]):
                entry["error"] = "a result differs: not timed"
                result["shapes"][name] = entry
                continue
            times = {"new": [], "new_hinted": [], "composition": []}
            for _ in range(args.rounds):
                for side, fn in (("new", lambda: run_new(kcol, length)), ("composition", lambda: run_composition(kcol, length)),
                                 ("new_hinted", lambda: run_new(kcol, length, distinct_keys))):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    out = fn()
                    ctx.synchronize()
                    times[side].append((time.perf_counter() - t0) * 1e3)
                    del out
            for side, ts in times.items():
                entry[side] = {"ms": [round(t, 3) for t in ts], "median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                               "rows_per_s": round(args.rows / (float(np.median(ts)) * 1e-3))}
            spread = entry["composition"]["max_ms"] - entry["composition"]["min_ms"]
            entry["composition_spread_ms"] = round(spread, 3)
            entry["speedup"] = round(entry["composition"]["median_ms"] / entry["new"]["median_ms"], 3)
            entry["ok"] = bool(entry["new"]["median_ms"] <= entry["composition"]["median_ms"] + spread)
            # streamed: one operator over the same rows in blocks; the plans its blocks took
            ctx.set_option("debug", 1)
            op = ch.LimitBy(np.uint64, length, ctx=ctx)
            with captured_stderr() as box:
                ctx.synchronize()
                t0 = time.perf_counter()
                total = 0
                for b in range(0, args.rows, args.block_rows):
                    _, p = op.filter_block(kcol, b, min(args.rows, b + args.block_rows))
                    total += p
                ctx.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
            op.close()
            ctx.set_option("debug", 0)
            plans = [ln.split("plan=")[1].split()[0] for ln in box["text"].splitlines() if "limit_by plan=" in ln]
            entry["streamed"] = {"ms": round(ms, 3), "blocks": len(plans), "rows_per_s": round(args.rows / (ms * 1e-3)), "passed": total,
                                 "passed_agrees": bool(total == passed), "plans": {p: plans.count(p) for p in sorted(set(plans))}}
            last = plans[-1] if plans else None
            if PLAN_BYTES.get(last):
                entry["streamed"]["algorithmic_bytes_per_row_of_last_plan"] = PLAN_BYTES[last]
                entry["streamed"]["algorithmic_bytes_per_s"] = round(args.rows * PLAN_BYTES[last] / (ms * 1e-3))
            result["shapes"][name] = entry
            print(f"{name}: new {entry['new']['median_ms']} ms (hinted {entry['new_hinted']['median_ms']}), composition {entry['composition']['median_ms']} ms, "
                  f"streamed {entry['streamed']['ms']} ms", file=sys.stderr, flush=True)
        del kcol
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
