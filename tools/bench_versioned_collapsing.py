#!/usr/bin/env python3
"""The VersionedCollapsing merge of K sorted runs against what stands next to it, on one build and in one process.

  versioned   versioned_collapsing_merge_rows([key, version], description, run_offsets, sign, check=False): the whole call
  collapsing  collapsing_merge_rows of the same keys and signs: the nearest operator, which emits at most two rows a group
  merge       merge_sorted_permutation of the same keys: the merge tree both sit on.  versioned - merge is what the new passes (sign check,
              heads, tile, carry, decide, offsets, emit) cost
  copy        chgpu_col_concat of a UInt8 column, repeated until it has read + written the versioned call's model bytes (below)

Shapes, --rows rows in total: (Int64 key, UInt32 version last in the description, Int8 sign) in K = 2, 8, 64 equal runs with about 1, 10
and 1000 rows per (key, version) group, under two sign mixes: `cancel` -- the runs of the first half hold state rows (+1) and those of
the second half their cancel rows (-1), so inside a group every + is followed later by a - -- and `positive` (nothing cancels, every row
is written).  The runs are made on the device (every run sorted in place by sort_block).  Before anything is timed the call is compared
with tests/versioned_collapsing_ref.py's vectorised form at --check-rows rows.  Then the sides run alternately, --rounds times after one
warm-up; a time is a host clock around synchronised work.  Model bytes: the merge tree's (merge_tree_bytes of csrc/merge_host.h, first
key 8 bytes) + per row the sign check 1, the heads 12 + 1, the tile pass 4 + 1 + 1 + 1/8, the decide pass 1 + 1/8 + 1/8, the emit pass
1/8 + 4 + per survivor 8.  `slower` marks where the whole call takes longer than Collapsing's by more than the ratio of their model
bytes.  --only LABEL runs one shape once without the other sides: the run to put under a kernel trace for per-kernel times.  One JSON
document on stdout, and in --out."""
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
MIXES = ("cancel", "positive")
SPEC = [(0, False, 1), (1, False, 1)]
NEW_PASS_BYTES_PER_ROW = 1 + 13 + (4 + 1 + 1 + 0.125) + (1 + 0.125 + 0.125) + (0.125 + 4)


def model_bytes(rows, n_runs, outputs):
    return int(merge_tree_bytes(8, rows, n_runs) + rows * NEW_PASS_BYTES_PER_ROW + 8 * outputs)


def collapsing_model_bytes(rows, n_runs, outputs):
    return int(merge_tree_bytes(8, rows, n_runs) + rows * (13 + 3 * (5 + 1)) + 8 * outputs)


def make_keys(rng, rows, per_group):
    """key, version: about per_group rows per pair"""
    return [rng.integers(0, max(1, rows // per_group // 2), size=rows, dtype=np.int64), rng.integers(0, 2, size=rows, dtype=np.uint32)]


def make_sign(mix, rows):
    sign = np.ones(rows, dtype=np.int8)
    if mix == "cancel":
        sign[rows // 2:] = -1       # K is even: a run holds one sign
    return sign


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10**8)
    ap.add_argument("--check-rows", type=int, default=10**6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", default="", help="a shape label such as cancel_k8_g10: that call alone, once after a warm-up")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import clickhouse_amd as ch
    import versioned_collapsing_ref as V
    if not torch.cuda.is_available():
        sys.exit("bench_versioned_collapsing: no GPU; nothing is measured without one")
    ctx = ch.Context(0)
    props = torch.cuda.get_device_properties(0)
    doc = {"bench": "versioned_collapsing", "rows": args.rows, "check_rows": args.check_rows, "rounds": args.rounds, "seed": args.seed,
           "gpu": {"name": props.name, "arch": getattr(props, "gcnArchName", "")}, "new_pass_bytes_per_row": NEW_PASS_BYTES_PER_ROW, "shapes": {}}
    rng = np.random.Generator(np.random.PCG64(args.seed))

    def sorted_runs(raw, k, rows):
        offs = [rows * r // k for r in range(k + 1)]
        parts = [[] for _ in raw]
        for r in range(k):
            block, _ = ch.sort_block([c.cut(offs[r], offs[r + 1] - offs[r]) for c in raw], SPEC)
            for j, c in enumerate(block):
                parts[j].append(c)
        return [ch.concat(p) for p in parts], offs

    if not args.only:
        # the check against the reference at --check-rows rows, every group size and mix, K = 8
        for per_group in GROUP_SIZES:
            keys, offs = sorted_runs([ctx.upload(c) for c in make_keys(rng, args.check_rows, per_group)], 8, args.check_rows)
            host = [c.numpy() for c in keys]
            d = [(host[0], False, 1), (host[1], False, 1)]
            for mix in MIXES:
                sign = make_sign(mix, args.check_rows)
                rows, balance = ch.versioned_collapsing_merge_rows(keys, SPEC, offs, sign, check=True)
                want_rows, want_balance = V.versioned_vector(d, sign)
                assert np.array_equal(rows.numpy(), want_rows) and balance == want_balance, f"{mix} differs at {per_group} rows per group"
            del keys
        doc["checked_against_reference"] = True

    chunk = 1 << 30
    copy_src = None if args.only else ctx.upload(np.zeros(chunk, dtype=np.uint8))

    def copy_side(nbytes):
        reps = max(1, int(round(nbytes / (2.0 * chunk))))

        def run():
            for _ in range(reps):
                ch.concat([copy_src])
        return run, reps * 2 * chunk

    for per_group in GROUP_SIZES:
        if args.only and not args.only.endswith(f"_g{per_group}"):
            continue
        raw = [ctx.upload(c) for c in make_keys(rng, args.rows, per_group)]
        for k in RUN_COUNTS:
            if args.only and f"_k{k}_" not in args.only:
                continue
            keys, offs = sorted_runs(raw, k, args.rows)
            merge = lambda: ch.merge_sorted_permutation(keys, SPEC, offs, check=False)   # noqa: E731
            for mix in MIXES:
                label = f"{mix}_k{k}_g{per_group}"
                if args.only and args.only != label:
                    continue
                sign = ctx.upload(make_sign(mix, args.rows))
                versioned = lambda: ch.versioned_collapsing_merge_rows(keys, SPEC, offs, sign, check=False)   # noqa: E731
                collapsing = lambda: ch.collapsing_merge_rows(keys, SPEC, offs, sign, check=False)            # noqa: E731
                out, balance = versioned()
                outputs = len(out)
                del out
                if args.only:
                    ms, res = timed(ctx, versioned)
                    del res
                    doc["shapes"][label] = {"runs": k, "rows_per_group": per_group, "mix": mix, "outputs": outputs, "max_balance": balance, "once_ms": round(ms, 3)}
                    continue
                collapsing_outputs = len(collapsing())
                nbytes = model_bytes(args.rows, k, outputs)
                collapsing_bytes = collapsing_model_bytes(args.rows, k, collapsing_outputs)
                copy_run, copy_bytes = copy_side(nbytes)
                sides = {"versioned": versioned, "collapsing": collapsing, "merge": merge, "copy": copy_run}
                times = {s: [] for s in sides}
                for rnd in range(args.rounds + 1):
                    for s, fn in sides.items():
                        ms, res = timed(ctx, fn)
                        del res
                        if rnd:
                            times[s].append(ms)
                entry = {"runs": k, "rows_per_group": per_group, "mix": mix, "outputs": outputs, "max_balance": balance, "model_bytes": nbytes,
                         "model_bytes_per_row": round(nbytes / args.rows, 3), "collapsing_outputs": collapsing_outputs, "collapsing_model_bytes": collapsing_bytes}
                for s in sides:
                    entry[s] = stats(times[s])
                entry["copy"]["bytes"] = copy_bytes
                entry["new_passes_ms"] = round(entry["versioned"]["median_ms"] - entry["merge"]["median_ms"], 3)
                entry["versioned_over_collapsing"] = round(entry["versioned"]["median_ms"] / entry["collapsing"]["median_ms"], 3)
                entry["versioned_over_copy"] = round(entry["versioned"]["median_ms"] / entry["copy"]["median_ms"], 3)
                entry["model_bytes_over_collapsing"] = round(nbytes / collapsing_bytes, 3)
                entry["slower"] = entry["versioned_over_collapsing"] > max(1.0, entry["model_bytes_over_collapsing"])
                doc["shapes"][label] = entry
                print(f"# {label}: versioned {entry['versioned']['median_ms']} ms, collapsing {entry['collapsing']['median_ms']} ms, merge "
                      f"{entry['merge']['median_ms']} ms, copy {entry['copy']['median_ms']} ms, outputs {outputs}, max_balance {balance}", file=sys.stderr, flush=True)
                del sign
            del keys
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
