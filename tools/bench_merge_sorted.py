#!/usr/bin/env python3
"""The merge of K sorted runs against what a caller had before it, on one build and in one process.

  merge      merge_sorted_permutation(keys, description, run_offsets, limit, check=False) + index of the key columns by it
  sort       sort_block(keys, description, limit) of the concatenation: the operator a caller has today (it sorts again from nothing)
  copy       chgpu_col_concat of a UInt8 column, repeated until it has read + written the bytes the plan's byte model says the merge
             moves (merge_tree_bytes / merge_sort_bytes of csrc/merge_host.h, restated in merge_bench_common.py and below): the time those bytes cost at copy speed
  check      is_sorted over the same runs (what check=True adds)

Shapes, --rows rows in total in K = 2, 8, 64, 1024 equal runs: Int64 keys; UInt8 keys; (UInt32 of 1000 distinct values, Int64), where
first-word ties are the rule; and LIMIT 10 at K = 8 for each.  The runs are made on the device: random columns are uploaded once per key
set and every run is sorted in place by sort_block.  Before anything is timed the merge's permutation is compared with sort_block's at
full size, and at --check-rows rows with numpy's stable lexsort.  Then the sides run alternately, --rounds times after one warm-up; a
time is a host clock around synchronised work.  `plan` is what merge_plan picks for the shape (tree / sort).  A ratio above 1 means
the merge is faster than sort_block; `slower` marks the shapes where it is not.  One JSON document on stdout, and in --out."""
import argparse
import json
import os
import sys

import numpy as np

from merge_bench_common import merge_tree_bytes, stats, timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

KEYSETS = {
    "int64": ([np.int64], [(0, False, 1)]),
    "uint8": ([np.uint8], [(0, False, 1)]),
    "uint32x1000_int64": ([np.uint32, np.int64], [(0, False, 1), (1, False, 1)]),
}
RUN_COUNTS = (2, 8, 64, 1024)


def model(key_sizes, rows, cut_rows, n_runs):
    """the tree's bytes, merge_sort_bytes and merge_plan of csrc/merge_host.h"""
    tree = merge_tree_bytes(key_sizes[0], cut_rows, n_runs)
    sort = rows * sum((s + 1) * 2 * (s + 8) for s in key_sizes)
    return tree, sort, "tree" if tree <= 2 * sort else "sort"   # MRG_SORT_BYTE_COST


def make_columns(rng, dtypes, rows):
    cols = []
    for k, dt in enumerate(dtypes):
        if dt == np.uint8:
            cols.append(rng.integers(0, 256, size=rows, dtype=np.uint8))
        elif dt == np.uint32:
            cols.append(rng.integers(0, 1000, size=rows, dtype=np.uint32))
        else:
            cols.append(rng.integers(-2**62, 2**62, size=rows, dtype=np.int64))
    return cols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10**8)
    ap.add_argument("--check-rows", type=int, default=10**6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    ap.add_argument("--keysets", default=",".join(KEYSETS), help="comma-separated subset of " + ", ".join(KEYSETS))
    ap.add_argument("--run-counts", default=",".join(str(k) for k in RUN_COUNTS), help="comma-separated run counts (the LIMIT 10 shape runs with 8)")
    args = ap.parse_args()
    keysets = {name: KEYSETS[name] for name in args.keysets.split(",")}
    run_counts = tuple(int(k) for k in args.run_counts.split(","))

    import torch

    import clickhouse_amd as ch
    if not torch.cuda.is_available():
        sys.exit("bench_merge_sorted: no GPU; nothing is measured without one")
    ctx = ch.Context(0)
    props = torch.cuda.get_device_properties(0)
    doc = {"bench": "merge_sorted", "rows": args.rows, "check_rows": args.check_rows, "rounds": args.rounds, "seed": args.seed,
           "gpu": {"name": props.name, "arch": getattr(props, "gcnArchName", "")}, "shapes": {}}
    rng = np.random.Generator(np.random.PCG64(args.seed))

    def sorted_runs(raw, spec, k, rows):
        """device columns whose k equal runs are each sorted by spec, and the run offsets"""
        offs = [rows * r // k for r in range(k + 1)]
        parts = [[] for _ in raw]
        for r in range(k):
            block, _ = ch.sort_block([c.cut(offs[r], offs[r + 1] - offs[r]) for c in raw], spec)
            for j, c in enumerate(block):
                parts[j].append(c)
        return [ch.concat(p) for p in parts], offs

    def merge_side(cols, spec, offs, limit):
        perm = ch.merge_sorted_permutation(cols, spec, offs, limit=limit, check=False)
        return [c.index(perm) for c in cols], perm

    # copy speed: one 1 GiB UInt8 column, copied `reps` times
    chunk = 1 << 30
    copy_src = ctx.upload(np.zeros(chunk, dtype=np.uint8))

    def copy_side(model_bytes):
        reps = max(1, int(round(model_bytes / (2.0 * chunk))))
        def run():
            for _ in range(reps):
                ch.concat([copy_src])
        return run, reps * 2 * chunk

    for name, (dtypes, spec) in keysets.items():
        key_sizes = [np.dtype(d).itemsize for d in dtypes]
        # the small check against numpy, K = 8 and 1024
        small = make_columns(rng, dtypes, args.check_rows)
        small_dev = [ctx.upload(c) for c in small]
        for k in (8, 1024):
            cols, offs = sorted_runs(small_dev, spec, k, args.check_rows)
            host = [c.numpy() for c in cols]
            want = np.lexsort([host[pos] for pos, _, _ in spec][::-1]).astype(np.uint64)
            got = ch.merge_sorted_permutation(cols, spec, offs, check=True).numpy()
            assert np.array_equal(got, want), f"{name} K={k}: the merge differs from numpy's stable lexsort at {args.check_rows} rows"
        del small_dev
        raw = [ctx.upload(c) for c in make_columns(rng, dtypes, args.rows)]
        for k, limit in [(k, 0) for k in run_counts] + ([(8, 10)] if 8 in run_counts else []):
            label = f"{name}_k{k}" + (f"_limit{limit}" if limit else "")
            cols, offs = sorted_runs(raw, spec, k, args.rows)
            cut_rows = sum(min(b - a, limit) if limit else b - a for a, b in zip(offs, offs[1:]))
            tree_b, sort_b, plan = model(key_sizes, args.rows, cut_rows, k)
            entry = {"keys": name, "runs": k, "limit": limit, "plan": plan, "model_tree_bytes": tree_b, "model_sort_bytes": sort_b}
            _, mperm = merge_side(cols, spec, offs, limit)
            _, sperm = ch.sort_block(cols, spec, limit)
            entry["sides_agree"] = bool(np.array_equal(mperm.numpy(), sperm.numpy()))
            assert entry["sides_agree"], f"{label}: the merge differs from sort_block of the concatenation"
            assert ch.is_sorted(cols, spec, offs) is None
            del mperm, sperm
            copy_run, copy_bytes = copy_side(tree_b if plan == "tree" else sort_b)
            sides = {"merge": lambda: merge_side(cols, spec, offs, limit), "sort": lambda: ch.sort_block(cols, spec, limit), "copy": copy_run,
                     "merge_perm_only": lambda: ch.merge_sorted_permutation(cols, spec, offs, limit=limit, check=False),
                     "check": lambda: ch.is_sorted(cols, spec, offs)}
            times = {s: [] for s in sides}
            for rnd in range(args.rounds + 1):
                for s, fn in sides.items():
                    ms, out = timed(ctx, fn)
                    del out
                    if rnd:
                        times[s].append(ms)
            for s in sides:
                entry[s] = stats(times[s])
            entry["copy"]["bytes"] = copy_bytes
            entry["copy"]["bytes_per_s"] = int(copy_bytes / (entry["copy"]["median_ms"] * 1e-3))
            entry["merge"]["model_bytes_per_s"] = int((tree_b if plan == "tree" else sort_b) / (entry["merge_perm_only"]["median_ms"] * 1e-3))
            entry["speedup_vs_sort"] = round(entry["sort"]["median_ms"] / entry["merge"]["median_ms"], 3)
            entry["merge_perm_over_copy"] = round(entry["merge_perm_only"]["median_ms"] / entry["copy"]["median_ms"], 3)
            entry["slower"] = entry["speedup_vs_sort"] < 1.0
            doc["shapes"][label] = entry
            print(f"# {label}: plan={plan} merge {entry['merge']['median_ms']} ms, sort {entry['sort']['median_ms']} ms, copy {entry['copy']['median_ms']} ms, "
                  f"perm only {entry['merge_perm_only']['median_ms']} ms, check {entry['check']['median_ms']} ms", file=sys.stderr, flush=True)
            del cols
        del raw
        ctx.trim()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
