#!/usr/bin/env python3
"""ORDER BY over a String column on the device: chgpu_string_sort_permutation (MSD sort in 8-byte words, every round the stable radix
passes of the numeric sort), chgpu_string_index and chgpu_string_filter by a 50 % random mask, HBM-resident inputs.  Next to every
case: the same number of rows sorted as a UInt64 column by chgpu_sort_permutation on the same build (the floor of a one-round sort: 8 passes against 9 plus the key gather), and a
one-core numpy stable argsort of the same values as a fixed-width byte dtype.
usage: bench_string_sort.py [rows]  -> one JSON object"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import clickhouse_amd as ch
from clickhouse_amd.lowcardinality import ColumnString

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
dev = torch.device("cuda", 0)
st = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(st)
ctx = ch.Context(0, st.cuda_stream)
g = torch.Generator(device=dev).manual_seed(7)
res = []


def best_of(fn, reps=3):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        del out
    return best


def fixed_width_column(body):
    """body: (rows, width) uint8 tensor of value bytes -> ColumnString of `rows` values of `width` bytes (+ the zero, + 64 bytes of pad)"""
    n, width = body.shape
    flat = torch.zeros(n * (width + 1) + 64, dtype=torch.uint8, device=dev)
    flat[:n * (width + 1)].view(n, width + 1)[:, :width] = body
    offs = torch.arange(1, n + 1, dtype=torch.int64, device=dev) * (width + 1)
    return ColumnString(ctx.wrap(offs.data_ptr(), np.uint64, n, keepalive=offs), ctx.wrap(flat.data_ptr(), np.uint8, n * (width + 1), keepalive=flat))


def random_bytes(n, width, lo=33, hi=127):
    return torch.randint(lo, hi, (n, width), dtype=torch.int32, device=dev, generator=g).to(torch.uint8)


def city_like(n, width):
    """'CITY-' + digits, 250 distinct values (SSB c_city / s_city), cut or padded to `width` bytes"""
    cid = torch.randint(0, 250, (n,), dtype=torch.int64, device=dev, generator=g)
    body = torch.full((n, 10), 48, dtype=torch.uint8, device=dev)
    for k, c in enumerate(b"CITY-"):
        body[:, k] = c
    # the value's two leading digits sit in bytes 5-6, its last digit in byte 9: 8 bytes do not tell all 250 values apart
    body[:, 5] = ((cid // 100) % 10 + 48).to(torch.uint8)
    body[:, 6] = ((cid // 10) % 10 + 48).to(torch.uint8)
    body[:, 9] = (cid % 10 + 48).to(torch.uint8)
    return body[:, :width].contiguous()


def url_like(n):
    body = torch.empty((n, 40), dtype=torch.uint8, device=dev)
    body[:, :24] = torch.tensor(list(b"https://www.example.com/"), dtype=torch.uint8, device=dev)
    body[:, 24:] = random_bytes(n, 16, 97, 123)
    return body


def words_of(body, k):
    w = torch.zeros(body.shape[0], dtype=torch.int64, device=dev)
    for c in range(8 * k, min(8 * k + 8, body.shape[1])):
        w = w * 256 + body[:, c].to(torch.int64)  # wraps for bytes >= 0x80 in the lead: still one number per word
    return w


def active_rows_per_round(body):
    """what the sort does with a fixed-width column whose values are decided after two words at most: the whole words all rows share
    are skipped, round 0 keys every row, round 1 keys the rows whose round-0 word is not unique"""
    n, width = body.shape
    skip = 0
    while 8 * (skip + 1) <= width and bool((body[:, 8 * skip:8 * skip + 8] == body[0, 8 * skip:8 * skip + 8]).all()):
        skip += 1
    if width <= 8 * (skip + 1):
        return [n]
    assert width <= 8 * (skip + 2)
    _, inverse, counts = torch.unique(words_of(body, skip), return_inverse=True, return_counts=True)
    again = int((counts[inverse] > 1).sum())
    return [n, again] if again else [n]


# the floor: the same number of rows as a UInt64 column through the numeric sort of the same build
t = torch.randint(-2**62, 2**62, (rows,), dtype=torch.int64, device=dev, generator=g)
col = ctx.wrap(t.data_ptr(), np.uint64, rows, keepalive=t)
u64_s = best_of(lambda: ch.sort_permutation(col, None, False, 1))
res.append({"case": "chgpu_sort_permutation UInt64 (floor)", "rows": rows, "ms": u64_s * 1e3, "rows_per_s": rows / u64_s})
del col, t

cases = [("8-byte distinct values", lambda: random_bytes(rows, 8)),
         ("10-byte city-like values, 250 distinct", lambda: city_like(rows, 10)),
         ("8-byte city-like values (round 0 of the case above alone)", lambda: city_like(rows, 8)),
         ("URL-like: 24-byte shared prefix + 16 random bytes", lambda: url_like(rows))]
for name, make in cases:
    body = make()
    width = body.shape[1]
    cs = fixed_width_column(body)
    active = active_rows_per_round(body)
    before = ctx.counters()["KernelLaunches"]
    perm = cs.get_permutation()
    launches = ctx.counters()["KernelLaunches"] - before
    # sorted order: neighbours in the result never decrease (checked on the first 8 bytes, big-endian, where that decides) and the
    # result is a permutation
    p = torch.from_numpy(perm.numpy().astype(np.int64)).to(dev)
    assert int(torch.bincount(p, minlength=rows).max()) == 1
    if width == 8:
        key = words_of(body, 0)
        assert bool((key[p][1:] >= key[p][:-1]).all())
        del key
    del p, perm
    dt = best_of(lambda: cs.get_permutation())
    dd = best_of(lambda: cs.get_permutation(None, True))
    dl = best_of(lambda: cs.get_permutation(None, False, 10))
    perm = cs.get_permutation()
    di = best_of(lambda: cs.index(perm))
    del perm
    # ColumnString.filter by a random mask that keeps half of the rows: 9 bytes per row (offset, mask byte), the kept values read and written
    keep = torch.rand(rows, device=dev, generator=g) < 0.5
    kept = int(keep.sum())
    mask8 = keep.to(torch.uint8)
    mask = ctx.wrap(mask8.data_ptr(), np.uint8, rows, keepalive=mask8)
    assert cs.filter(mask).size() == kept
    df = best_of(lambda: cs.filter(mask))
    del mask, mask8, keep
    m = min(rows, 5_000_000)
    host = body[:m].cpu().numpy().copy().view(f"S{width}").reshape(m)
    t0 = time.perf_counter(); np.argsort(host, kind="stable"); tc = time.perf_counter() - t0
    res.append({"case": name, "rows": rows, "value_bytes": width, "active_rows_per_round": active, "kernel_launches": launches,
                "ms": dt * 1e3, "ms_per_active_Mrow": dt * 1e3 / (sum(active) / 1e6), "ms_descending": dd * 1e3, "ms_limit_10": dl * 1e3, "rows_per_s": rows / dt,
                "ratio_to_uint64_sort": dt / u64_s, "ratio_to_uint64_sort_per_active_row": dt / (sum(active) / rows) / u64_s,
                "string_index_by_the_permutation_ms": di * 1e3, "string_index_GBps": (2 * (width + 1) + 32) * rows / di / 1e9,
                "string_filter_half_ms": df * 1e3, "string_filter_half_GBps": (2 * (width + 1) * kept + 9 * rows) / df / 1e9,
                "cpu_numpy_stable_argsort_rows_per_s_1thread": m / tc, "cpu_sample_rows": m, "speedup_over_numpy_1thread": (rows / dt) / (m / tc)})
    del cs, body
    ctx.trim()
    torch.cuda.empty_cache()
print(json.dumps({"results": res}))
