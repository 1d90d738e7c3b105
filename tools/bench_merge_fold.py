#!/usr/bin/env python3
"""The folding merges (Replacing, Collapsing, Summing) of K sorted runs against what a caller has without them, on one build and in one
process.

  fold       replacing_merge_rows / collapsing_merge_rows / summing_merge_rows(keys, description, run_offsets, .., check=False)
  merge      merge_sorted_permutation of the same keys: the floor the fold sits on (it runs the same merge tree first)
  copy       chgpu_col_concat of a UInt8 column, repeated until it has read + written the fold's model bytes (below)
  hash       Replacing and Summing only: the hash aggregator's argMax(row, version) / sum GROUP BY of the same rows, finalised.  It
             answers in table order, so a caller would still have to sort its result; that sort is not timed.

Shapes, --rows rows in total: (Int64 key, UInt64 version | Int8 sign | two UInt64 values) in K = 2, 8, 64 equal runs with about 1, 10
and 1000 rows per group.  The runs are made on the device (every run sorted in place by sort_block).  Before anything is timed each
algorithm is compared with tests/merge_fold_ref.py's vectorised form at --check-rows rows.  Then the sides run alternately, --rounds times
after one warm-up; a time is a host clock around synchronised work.  `slower` marks where the fold loses to the hash aggregator.  Model
bytes: the merge tree's (merge_tree_bytes of csrc/merge_host.h) + per row the heads (12 + 1) and three passes over (flag 1, row 4, the
gathered argument bytes) + per output the row numbers (8 each) and the result widths.  One JSON document on stdout, and in --out."""
import argparse
import json
import os
import sys

import numpy as np

from merge_bench_common import merge_tree_bytes, stats, timed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

RUN_COUNTS = (2, 8, 64)
GROUP_SIZES = (1, 10, 1000)
SPEC = [(0, False, 1)]
ARG_BYTES = {"replacing": 8, "collapsing": 1, "summing": 16}


def model_bytes(algo, rows, n_runs, outputs):
    out = outputs * (8 + 8 + 16 if algo == "summing" else 8)
    return merge_tree_bytes(8, rows, n_runs) + rows * (13 + 3 * (5 + ARG_BYTES[algo])) + out


def make_columns(rng, rows, per_group):
    """key, version, sign, value a, value b"""
    return [rng.integers(0, max(1, rows // per_group), size=rows, dtype=np.int64), rng.integers(0, 4, size=rows, dtype=np.uint64),
            np.where(rng.integers(0, 2, size=rows, dtype=np.int8) == 1, 1, -1).astype(np.int8), rng.integers(0, 2**40, size=rows, dtype=np.uint64),
            rng.integers(0, 3, size=rows, dtype=np.uint64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10**8)
    ap.add_argument("--check-rows", type=int, default=10**6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import clickhouse_amd as ch
    import merge_fold_ref as F
    from clickhouse_amd import _capi as K
    if not torch.cuda.is_available():
        sys.exit("bench_merge_fold: no GPU; nothing is measured without one")
    ctx = ch.Context(0)
    props = torch.cuda.get_device_properties(0)
    doc = {"bench": "merge_fold", "rows": args.rows, "check_rows": args.check_rows, "rounds": args.rounds, "seed": args.seed,
           "gpu": {"name": props.name, "arch": getattr(props, "gcnArchName", "")}, "shapes": {}}
    rng = np.random.Generator(np.random.PCG64(args.seed))

    def sorted_runs(raw, k, rows):
        offs = [rows * r // k for r in range(k + 1)]
        parts = [[] for _ in raw]
        for r in range(k):
            block, _ = ch.sort_block([c.cut(offs[r], offs[r + 1] - offs[r]) for c in raw], SPEC)
            for j, c in enumerate(block):
                parts[j].append(c)
        return [ch.concat(p) for p in parts], offs

    def fold_sides(cols, offs):
        key, version, sign, a, b = cols
        return {"replacing": lambda: ch.replacing_merge_rows([key], SPEC, offs, version, check=False),
                "collapsing": lambda: ch.collapsing_merge_rows([key], SPEC, offs, sign, check=False),
                "summing": lambda: ch.summing_merge_rows([key], SPEC, offs, [a, b], check=False)}

    # the check against the reference at --check-rows rows, every group size, K = 8
    for per_group in GROUP_SIZES:
        cols, offs = sorted_runs([ctx.upload(c) for c in make_columns(rng, args.check_rows, per_group)], 8, args.check_rows)
        host = [c.numpy() for c in cols]
        d = [(host[0], False, 1)]
        sides = fold_sides(cols, offs)
        assert np.array_equal(sides["replacing"]().numpy(), F.replacing_vector(d, host[1])), f"replacing differs at {per_group} rows per group"
        assert np.array_equal(sides["collapsing"]().numpy(), F.collapsing_vector(d, host[2])), f"collapsing differs at {per_group} rows per group"
        first, last, res = sides["summing"]()
        want = F.folding_vector(d, [host[3], host[4]], ["sum", "sum"], True)
        assert np.array_equal(first.numpy(), want[0]) and np.array_equal(last.numpy(), want[1]), f"summing differs at {per_group} rows per group"
        assert all(np.array_equal(r.numpy(), w) for r, w in zip(res, want[2])), f"summing differs at {per_group} rows per group"
        del cols, sides, first, last, res
    doc["checked_against_reference"] = True

    chunk = 1 << 30
    copy_src = ctx.upload(np.zeros(chunk, dtype=np.uint8))
    row_ids = ctx.upload(np.arange(args.rows, dtype=np.uint64))

    def copy_side(nbytes):
        reps = max(1, int(round(nbytes / (2.0 * chunk))))

        def run():
            for _ in range(reps):
                ch.concat([copy_src])
        return run, reps * 2 * chunk

    def hash_side(algo, cols, groups):
        key, version, _, a, b = cols
        if algo == "replacing":
            def run():
                agg = ch.Aggregator(np.int64, [(K.AGG_ARG_MAX, (np.uint64, np.uint64))], size_hint=groups, ctx=ctx)
                agg.execute_on_block(key, [(row_ids, version)])
                out = agg.finalize_columns()
                agg.close()
                return out
            return run

        def run():
            agg = ch.Aggregator(np.int64, [(K.AGG_SUM, np.uint64), (K.AGG_SUM, np.uint64)], size_hint=groups, ctx=ctx)
            agg.execute_on_block(key, [a, b])
            out = agg.finalize_columns()
            agg.close()
            return out
        return run

    for per_group in GROUP_SIZES:
        raw = [ctx.upload(c) for c in make_columns(rng, args.rows, per_group)]
        for k in RUN_COUNTS:
            cols, offs = sorted_runs(raw, k, args.rows)
            folds = fold_sides(cols, offs)
            merge = lambda: ch.merge_sorted_permutation([cols[0]], SPEC, offs, check=False)   # noqa: E731
            for algo, fold in folds.items():
                label = f"{algo}_k{k}_g{per_group}"
                out = fold()
                outputs = len(out[0] if algo == "summing" else out)
                del out
                nbytes = model_bytes(algo, args.rows, k, outputs)
                copy_run, copy_bytes = copy_side(nbytes)
                sides = {"fold": fold, "merge": merge, "copy": copy_run}
                if algo != "collapsing":
                    sides["hash"] = hash_side(algo, cols, max(1, args.rows // per_group))
                times = {s: [] for s in sides}
                for rnd in range(args.rounds + 1):
                    for s, fn in sides.items():
                        ms, res = timed(ctx, fn)
                        del res
                        if rnd:
                            times[s].append(ms)
                entry = {"algorithm": algo, "runs": k, "rows_per_group": per_group, "outputs": outputs, "model_bytes": nbytes}
                for s in sides:
                    entry[s] = stats(times[s])
                entry["copy"]["bytes"] = copy_bytes
                entry["fold_over_merge"] = round(entry["fold"]["median_ms"] / entry["merge"]["median_ms"], 3)
                entry["fold_over_copy"] = round(entry["fold"]["median_ms"] / entry["copy"]["median_ms"], 3)
                if "hash" in entry:
                    entry["speedup_vs_hash"] = round(entry["hash"]["median_ms"] / entry["fold"]["median_ms"], 3)
                    entry["slower"] = entry["speedup_vs_hash"] < 1.0
                doc["shapes"][label] = entry
                print(f"# {label}: fold {entry['fold']['median_ms']} ms, merge {entry['merge']['median_ms']} ms, copy {entry['copy']['median_ms']} ms"
                      + (f", hash {entry['hash']['median_ms']} ms" if "hash" in entry else "") + f", outputs {outputs}", file=sys.stderr, flush=True)
            del cols, folds
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
