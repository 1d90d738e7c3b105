"""What the three merge benchmarks (bench_merge_sorted.py, bench_merge_fold.py, bench_versioned_collapsing.py) share: the merge
tree's model bytes, the host clock around synchronised work and the summary of a side's times."""
import time


def round_count(k):
    """merge_round_count of csrc/merge_host.h: the rounds of the pairwise tree over k runs"""
    t, n = 0, 1
    while n < k:
        n, t = n * 2, t + 1
    return t


def merge_tree_bytes(first_key_size, cut_rows, n_runs):
    """merge_tree_bytes of csrc/merge_host.h: the key build reads the first column and writes a (u64 word, u32 row) pair, every round
    reads and writes the pair, the last step reads the row and writes the u64 permutation"""
    return cut_rows * (first_key_size + 12 + 24 * round_count(n_runs) + 12)


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    ms = sorted(ms)
    return {"ms": [round(x, 3) for x in ms], "median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3)}
