#!/usr/bin/env python3
"""bench.py — BASELINE.json's headline metric on MI355X: rows/sec (+ achieved HBM GB/s) of the block-processing hot path.

Workload at every N: BASELINE.json configs[1] — `SELECT sum(a), count() FROM t WHERE a < 214748365` (~10 % pass) over
1 000 000 000 Int64 rows per GPU, uniform [0, 2^31), resident in HBM before the timed region (synthetic, generated on
device).  One "step" = one pass of the fused HIP filter+sum kernel over the whole column plus the no-key state merge
(mergeWithoutKeyDataImpl): at N>1 every rank scans its own 1 B rows (weak scaling, no data-path collective) and the
16-byte {sum,count} states are summed with one RCCL all-reduce per step, issued asynchronously.

Contract: `python bench.py --gpus N --steps K --warmup W`; N>1 is launched by torch.distributed.run (one rank per GPU).
Rank 0 prints ONE JSON line.  `--dump-outputs DIR` also writes the result of the last timed step under DIR (inputs are seeded, so two
builds can be compared output for output).

A plain run does only what the headline needs: input, warm-up, timed steps, the line.  `--full` adds everything else the line has
carried: the headline checked against a torch recomputation, the CPU baselines, and the other configs on the same clock (N=1: C3,
C4, C5, Q11, C2 from host Blocks; N>1 or --force-dist: the sharded GROUP BY, join and SSB plan).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

THRESHOLD = 214748365  # ~10.0 % of uniform [0, 2^31)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000_000, help="rows per GPU (default: the 1 B rows of configs[1])")
    ap.add_argument("--full", action="store_true", help="after the headline, also run its reference check, the CPU baselines and the other "
                                                         "configs (the options below that say --full choose among these)")
    ap.add_argument("--cpu-sample-rows", type=int, default=1_000_000_000, help="--full: rows of the headline's CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-configs", action="store_true", help="--full: skip the configs sections of the line")
    ap.add_argument("--c3-rows", type=int, default=1_000_000_000)
    ap.add_argument("--c4-probe-rows", type=int, default=100_000_000)
    ap.add_argument("--c4-build-rows", type=int, default=10_000_000)
    ap.add_argument("--no-c5", action="store_true", help="--full: skip the SSB Q4.1-style section (configs[4], one GPU's share)")
    ap.add_argument("--c5-rows", type=int, default=750_000_000)
    ap.add_argument("--only-c5", action="store_true", help="--full: of the configs, run only C5 (the profile of the SSB plan on its own: profiles/collect.sh)")
    ap.add_argument("--sharded-timeout", type=float, default=240.0, help="--full, N>1: seconds the sharded GROUP BY / join section may take before the line is printed without it")
    ap.add_argument("--force-dist", action="store_true", help="initialise the process group even at world size 1 (exercises the RCCL code path on one GPU)")
    ap.add_argument("--backend", default="nccl", help="nccl (= RCCL, the measured configuration) or gloo (rehearsal of the N>1 code path on one GPU)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the {sum, count} state of the last timed step as DIR/<name>.npy (float64), "
                                                          "to compare two builds output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.only_c5 and not args.full:
        ap.error("--only-c5 chooses among the --full sections: give --full too")

    # the hosts of this pool only support dmabuf IPC: without it RCCL's peer buffers fail with hipIpcGetMemHandle: invalid argument.
    # Exported by the launch environment already; set before HIP starts in case a launcher drops it
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    import numpy as np
    import torch

    import clickhouse_amd as ch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N>1 must be launched with torch.distributed.run --nproc-per-node N")
        args.gpus = world
    if args.backend != "nccl":
        local_rank = local_rank % max(1, torch.cuda.device_count())  # rehearsal only: ranks may share a GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    _saved_stdout_fd = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")  # --force-dist without a launcher
        # stdout carries exactly one JSON line: RCCL prints its version banner to stdout when the communicator is created
        # (NCCL_DEBUG=VERSION is exported on the GPU boxes), so fd 1 points at stderr until the result is printed
        sys.stdout.flush()
        _saved_stdout_fd = os.dup(1)
        os.dup2(2, 1)
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)

    n = args.rows
    K, W = args.steps, args.warmup

    # ---- synthetic input, resident in HBM ----
    g = torch.Generator(device=dev).manual_seed(1 + rank)
    a = torch.randint(0, 2**31, (n,), dtype=torch.int64, device=dev, generator=g)
    results = torch.zeros((K + W, 2), dtype=torch.int64, device=dev)  # one {sum, count} state slot per step
    torch.cuda.synchronize()

    # the C-ABI context launches on this torch stream so the HIP events below bracket exactly its kernels
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    assert stream.cuda_stream != 0
    ctx = ch.Context(local_rank, stream.cuda_stream)
    col = ctx.wrap(a.data_ptr(), np.int64, n, keepalive=a)
    slots = [ctx.wrap(results[i].data_ptr(), np.uint64, 2, keepalive=results) for i in range(K + W)]

    works = []

    def merge_states(i):
        """mergeWithoutKeyDataImpl across ranks: one 16-byte all-reduce, asynchronous under RCCL"""
        if dist is None:
            return
        if args.backend == "nccl":
            works.append(dist.all_reduce(results[i], op=dist.ReduceOp.SUM, async_op=True))
        else:  # gloo rehearsal: stage through the host
            stream.synchronize()
            h = results[i].cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            results[i].copy_(h)

    def step(i):
        ch.filter_sum_async(col, ch.LT, THRESHOLD, None, slots[i])  # HIP kernels via the C ABI, no host sync
        merge_states(i)

    for i in range(W):
        step(i)
    for w in works:
        w.wait()
    works.clear()
    torch.cuda.synchronize()

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)]
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(K):
        ev[i][0].record(stream)
        ch.filter_sum_async(col, ch.LT, THRESHOLD, None, slots[W + i])
        ev[i][1].record(stream)
        merge_states(W + i)
    for w in works:
        w.wait()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    kern_ms = [s.elapsed_time(e) for s, e in ev]  # HIP events on the launch stream: filter+sum kernel (+ its 1-block finish)
    kern_avg_ms = sum(kern_ms) / len(kern_ms)

    if dist is not None:
        red_dev = dev if args.backend == "nccl" else "cpu"
        t = torch.tensor([elapsed, kern_avg_ms], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)  # MAX over ranks
        elapsed, kern_avg_ms = float(t[0].item()), float(t[1].item())

    # ---- sanity: every step produced the same state, with --full also the correct one (checked outside the timed region) ----
    res = results.cpu().numpy()
    assert (res == res[W]).all(), "steps disagree"
    if args.full and world == 1:
        want_sum = int(a[a < THRESHOLD].sum().item())
        want_cnt = int((a < THRESHOLD).sum().item())
        assert (int(res[W][0]), int(res[W][1])) == (want_sum, want_cnt), (res[W], want_sum, want_cnt)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, res[W + K - 1], np)

    total_rows = n * world * K
    value = total_rows / elapsed
    algo_bytes = 8.0 * n  # 8 B/row, one launch scans the rank's whole column
    achieved = algo_bytes / (kern_avg_ms * 1e-3) / 1e9

    # HBM bytes per launch from the PMC passes of THIS command (profiles/collect.sh writes the file; counters cannot be read
    # from inside the process, so the number is the last committed collection and traffic_source says which one)
    traffic, traffic_source, tj = None, None, {}
    tpath = os.path.join(REPO, "profiles", "traffic.json")
    if os.path.exists(tpath):
        try:
            tj = json.load(open(tpath))
            if tj.get("rows") == n:
                traffic = tj.get("k_filter_sum_hbm_bytes_per_launch")
                traffic_source = tj.get("source", "profiles/traffic.json")
        except Exception:
            traffic, tj = None, {}

    out = {
        "metric": json.load(open(os.path.join(REPO, "BASELINE.json")))["metric"],
        "value": value,
        "unit": "rows/s",
        "n_gpus": world,
        "steps": K,
        "warmup": W,
        "ms_per_step": elapsed / K * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic",
        "config": {
            "workload": "BASELINE.json configs[1]: SELECT sum(a), count() WHERE a < 214748365 (~10% pass) over Int64 rows, "
                        "HBM-resident, fused HIP filter+sum kernel",
            "rows_per_gpu": n,
            "global_rows_per_step": n * world,
            "parallelism": f"row-range shards x{world}, 16-byte state all-reduce" if world > 1 else "single GPU",
        },
        "roofline": {
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic,
            "traffic_source": traffic_source,
            "kernel": "k_filter_sum<long,2,true,false,IntRangePred>",
            "kernel_avg_ms": kern_avg_ms,
            "algorithmic_bytes_per_launch": algo_bytes,
        },
    }

    def emit(line):
        if rank == 0:
            nonlocal _saved_stdout_fd
            if _saved_stdout_fd is not None:
                sys.stdout.flush()
                os.dup2(_saved_stdout_fd, 1)  # the real stdout is back for the one JSON line
                os.close(_saved_stdout_fd)
                _saved_stdout_fd = None
            print(json.dumps(line), flush=True)
            if dist is not None:
                os.dup2(2, 1)  # anything RCCL says while shutting down goes to stderr again

    if not args.full:
        emit(out)
        if dist is not None:
            dist.destroy_process_group()
        return

    if world == 1 and dist is None:
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(a, args.cpu_sample_rows, ctx, ch)
        if not args.no_configs:
            # BASELINE.json configs[2] and configs[3] (its one-GPU half) on the same clock; `value` above stays configs[1]
            del a, col, slots, results
            ctx.trim()
            torch.cuda.empty_cache()
            out["configs"] = {}
            if not args.only_c5:
                out["configs"]["C3"] = config_c3(args, ctx, ch, torch, np, dev, stream, tj, not args.no_cpu_baseline)
                ctx.trim()
                torch.cuda.empty_cache()
                out["configs"]["C4_one_gpu"] = config_c4(args, ctx, ch, torch, np, dev, stream, tj, not args.no_cpu_baseline)
                ctx.trim()
                torch.cuda.empty_cache()
            if not args.no_c5:
                try:
                    out["configs"]["C5_one_gpu_share"] = config_c5(args, ctx, ch, torch, np, dev, stream, not args.no_cpu_baseline)
                except Exception as e:  # noqa: BLE001 -- the wider plan must not cost the headline line
                    out["configs"]["C5_one_gpu_share"] = {"error": f"{type(e).__name__}: {e}"[:400]}
                ctx.trim()
                torch.cuda.empty_cache()
            if not args.only_c5:
                for name, fn in (("Q11", config_q11), ("C2_from_host_blocks", config_c2_from_host_blocks)):
                    try:
                        out["configs"][name] = fn(args, ctx, ch, torch, np, dev, stream, not args.no_cpu_baseline, out.get("cpu_baseline"))
                    except Exception as e:  # noqa: BLE001
                        out["configs"][name] = {"error": f"{type(e).__name__}: {e}"[:400]}
                    ctx.trim()
                    torch.cuda.empty_cache()
        emit(out)
        return

    # ---- N > 1 (or --force-dist): the sharded GROUP BY and hash join, exchange over RCCL through the C ABI (chgpu_all_to_all) ----
    if not args.no_configs:
        del a, col, slots, results
        ctx.trim()
        torch.cuda.empty_cache()
        # The headline line must survive whatever the exchange does on hardware this build has never seen: if the sharded section has
        # not finished in time, every rank gives up on it, rank 0 prints the line without it and the process ends.
        import threading

        def give_up():
            out["configs"] = {"error": f"sharded section did not finish within {args.sharded_timeout} s"}
            emit(out)
            os._exit(3)  # the headline is on stdout, but a hung exchange must show in the driver's return code

        watchdog = threading.Timer(args.sharded_timeout, give_up)
        watchdog.daemon = True
        watchdog.start()
        try:
            out["configs"] = sharded_configs(args, ctx, ch, torch, np, dev, stream, rank, world, dist)
        except Exception as e:  # noqa: BLE001 -- reported in the line, the headline stays
            out["configs"] = {"error": f"{type(e).__name__}: {e}"[:500]}
        watchdog.cancel()
    emit(out)
    dist.destroy_process_group()


def sharded_configs(args, ctx, ch, torch, np, dev, stream, rank, world, dist):
    """BASELINE.json configs[2] and [3] across `world` GPUs: every rank holds its share of the rows; partial GROUP BY states and join
    rows are routed by key hash (owner = two-level bucket & (world - 1)) with chgpu_partition_by_hash + ONE chgpu_all_to_all per column
    over RCCL / xGMI; owners merge / build / probe locally.  torch.distributed is only the control plane here (id broadcast, barriers,
    the MAX over ranks of the timings)."""
    from clickhouse_amd import distributed as D

    def bcast(obj):
        box = [obj]
        dist.broadcast_object_list(box, src=0)
        return box[0]

    def max_over_ranks(x):
        backend_dev = dev if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([x], dtype=torch.float64, device=backend_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t[0].item())

    torch.cuda.synchronize()
    rehearsal = dist.get_backend() != "nccl"
    comm = _HostStagedComm(ctx, rank, world, dist, torch, np) if rehearsal else D.Comm.from_env(ctx, rank, world, bcast)
    eng = D.LocalEngine(ctx, comm)
    res = {}

    def timed(fn, reps=3, warmup=1):
        out_ = None
        for _ in range(warmup):
            out_ = fn()
        best = []
        for _ in range(reps):
            ctx.synchronize()
            dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out_ = fn()
            ctx.synchronize()
            best.append(max_over_ranks(time.perf_counter() - t0))
        return sum(best) / len(best), out_

    # ---- C3 sharded: every rank aggregates its own rows; partial states travel to their owners ------------------------------
    rows = args.c3_rows
    g = torch.Generator(device=dev).manual_seed(2 + 1000 * rank)
    k = torch.randint(0, 1_000_000, (rows,), dtype=torch.int32, device=dev, generator=g)
    v = torch.randint(-2**31, 2**31, (rows,), dtype=torch.int64, device=dev, generator=g)
    kc = ctx.wrap(k.data_ptr(), np.uint32, rows, keepalive=k)
    vc = ctx.wrap(v.data_ptr(), np.int64, rows, keepalive=v)
    aggs = [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)]

    def run_c3():
        sg = D.ShardedGroupBy(eng, np.uint32, aggs, size_hint=1_000_000)
        sg.add_block(kc, [vc, None])
        return sg, sg.finish_columns()

    before = comm.stats()
    secs, (sg, owner) = timed(run_c3)
    after = comm.stats()
    gk, (gs, gc) = owner.convert_to_block()
    # every group lives on exactly one rank, counts partition all rows, sums add up to the sum of all values (mod 2^64)
    sel = ch.hash_to_selector(ctx.upload(gk), world).numpy() if gk.shape[0] else np.zeros(0, dtype=np.uint32)
    assert (sel == rank).all(), "a rank holds groups it does not own"
    tot = comm.all_reduce_u64([gk.shape[0], int(gc.sum()), int(gs.astype(np.uint64).sum(dtype=np.uint64)), int(v.sum().item()) % 2**64])
    assert tot[1] == rows * world and tot[2] == tot[3], "sharded GROUP BY lost or duplicated rows"
    res["C3_sharded"] = {"workload": "GROUP BY UInt32 key (1 M groups), sum(Int64) + count(): local pre-aggregation, partial states routed by "
                                     "key hash with one all-to-all (RCCL), owner-side merge", "rows_per_gpu": rows, "global_rows": rows * world,
                         "groups": tot[0], "ms": secs * 1e3, "rows_per_s": rows * world / secs, "scaling": "weak",
                         "exchange_bytes_sent_per_rank": (after["bytes_sent"] - before["bytes_sent"]) // 4,
                         "parity": "groups owned by exactly one rank; counts partition the rows; sum of sums == sum of values (mod 2^64)"}
    if world == 1:
        A = ch.Aggregator(np.uint32, aggs, size_hint=1_000_000, ctx=ctx)
        A.execute_on_block(kc, [vc, None])
        ok_, (os_, oc_) = A.convert_to_block()
        i, j = np.argsort(gk), np.argsort(ok_)
        assert np.array_equal(gk[i], ok_[j]) and np.array_equal(gs[i], os_[j]) and np.array_equal(gc[i], oc_[j])
        res["C3_sharded"]["parity"] += "; world 1: equal to the single-GPU operator bit for bit"
        del A
    del k, v, kc, vc, sg, owner
    ctx.trim()
    torch.cuda.empty_cache()

    # ---- C4 sharded: configs[3]'s per-GPU share (1/8 of 100 M probe rows and of 10 M build rows per rank) -----------------------
    nb_all, np_all = args.c4_build_rows, args.c4_probe_rows
    share = 8
    nb_r, np_r = nb_all // share, np_all // share
    nb_tot, np_tot = nb_r * world, np_r * world
    g = torch.Generator(device=dev).manual_seed(5)   # the SAME table on every rank; a rank owns a slice of its rows
    bk = (torch.randperm(nb_tot, device=dev, generator=g).to(torch.int64) + 1) * 2654435761
    bv = torch.randint(-2**40, 2**40, (nb_tot,), dtype=torch.int64, device=dev, generator=g)
    pk = torch.where(torch.rand(np_tot, device=dev, generator=g) < 0.5, bk[torch.randint(0, nb_tot, (np_tot,), device=dev, generator=g)],
                     torch.randint(0, 2**62, (np_tot,), dtype=torch.int64, device=dev, generator=g))
    my_bk, my_bv = bk[rank * nb_r:(rank + 1) * nb_r].contiguous(), bv[rank * nb_r:(rank + 1) * nb_r].contiguous()
    my_pk = pk[rank * np_r:(rank + 1) * np_r].contiguous()
    bkc = ctx.wrap(my_bk.data_ptr(), np.uint64, nb_r, keepalive=my_bk)
    bvc = ctx.wrap(my_bv.data_ptr(), np.int64, nb_r, keepalive=my_bv)
    pkc = ctx.wrap(my_pk.data_ptr(), np.uint64, np_r, keepalive=my_pk)

    def build():
        j = D.ShardedHashJoin(eng, ch.JOIN_INNER, ch.STRICT_ALL)
        j.add_build_rows(bkc, [bvc])
        j.finish_build()
        return j

    before = comm.stats()
    b_secs, j = timed(build)
    p_secs, (cnt, sm) = timed(lambda: j.probe_count_sum(pkc, 0))
    after = comm.stats()
    # the same probe cut in two: routing (hash -> selector -> stable partition -> the exchange) and the join on the rows that landed here
    r_secs, (routed, _) = timed(lambda: j._route(pkc, []))
    l_secs, _ = timed(lambda: eng.join_count_sum(j.join, routed, j.payload[0]))
    sbk, order = torch.sort(bk)
    pos = torch.searchsorted(sbk, pk).clamp_(max=nb_tot - 1)
    hit = sbk[pos] == pk
    want = (int(hit.sum().item()), int(bv[order[pos[hit]]].sum().item()) % 2**64)
    assert (cnt, sm) == want, ("C4 sharded", cnt, sm, want)
    res["C4_sharded"] = {"workload": "probe INNER JOIN build on UInt64, SELECT count(), sum(bv): build and probe rows routed to the owner of "
                                     "their key with one all-to-all each (RCCL), joined where they land, 16-byte all-reduce of the aggregate; "
                                     "per-GPU share of configs[3] (1/8 of 100 M probe, 10 M build rows)",
                         "build_rows_per_gpu": nb_r, "probe_rows_per_gpu": np_r, "global_build_rows": nb_tot, "global_probe_rows": np_tot,
                         "matches": cnt, "build_ms": b_secs * 1e3, "probe_ms": p_secs * 1e3, "ms": (b_secs + p_secs) * 1e3,
                         "probe_route_and_exchange_ms": r_secs * 1e3, "probe_local_join_ms": l_secs * 1e3,
                         "rows_per_s": (nb_tot + np_tot) / (b_secs + p_secs), "scaling": "weak",
                         "exchange_bytes_sent_per_rank": (after["bytes_sent"] - before["bytes_sent"]) // 4,
                         "parity": "count and sum(payload) equal to an independent sorted-search join over the whole tables"}
    if world == 1:
        one = ch.HashJoin(ch.JOIN_INNER, ch.STRICT_ALL, ctx=ctx)
        one.add_block(bkc)
        c1, s1 = one.probe_count_sum(pkc, bvc)
        assert (c1, s1 % 2**64) == (cnt, sm)
        res["C4_sharded"]["parity"] += "; world 1: equal to the single-GPU operator bit for bit"
    del j, bk, bv, pk, my_bk, my_bv, my_pk, bkc, bvc, pkc
    ctx.trim()
    torch.cuda.empty_cache()

    # ---- C5 sharded: BASELINE.json configs[4] -- every rank holds rows/8 x ... its share of lineorder, the dimensions are replicated --------
    if not args.no_c5:
        sys.path.insert(0, os.path.join(REPO, "tools"))
        import ssb
        rows5 = args.c5_rows
        C5, S5, P5 = 30_000_000, 2_000_000, 2_000_000
        dims = ssb.gen_dims(C5, S5, P5)
        lo_t = ssb.gen_lineorder_torch(rows5, C5, S5, P5, dev, seed=11 + 1000 * rank)
        torch.cuda.synchronize()
        lo = {k_: ctx.wrap(v_.data_ptr(), np.uint32, rows5, keepalive=v_) for k_, v_ in lo_t.items()}
        dims_dev = ssb.upload_dims(ctx, dims)
        before = comm.stats()
        secs5, mine = timed(lambda: ssb.q41_sharded_gpu(ch, D, eng, dims_dev, lo))
        after = comm.stats()
        local = ssb.q41_gpu(ch, ctx, dims_dev, lo)   # this rank's rows through the one-GPU plan: an independent merge path for the check
        tot_owned = comm.all_reduce_u64([len(mine), sum(c_ for _, c_ in mine.values()), sum(p_ for p_, _ in mine.values()) % 2**64])
        tot_local = comm.all_reduce_u64([sum(c_ for _, c_ in local.values()), sum(p_ for p_, _ in local.values()) % 2**64])
        assert tot_owned[1] == tot_local[0] and tot_owned[2] == tot_local[1], "C5 sharded: owner-merged groups differ from the sum of the ranks' own results"
        assert tot_owned[0] == 35, ("C5 sharded: groups", tot_owned[0])
        res["C5_sharded"] = {"workload": "SSB Q4.1-style: lineorder sharded by row range, dimension tables replicated, every rank answers the four joins as one "
                                         "filter over its fact keys (chgpu_join_probe_chain), gathers the survivors and pre-aggregates; the (year, nation) "
                                         "partial states are routed to their owners in one exchange (RCCL) and merged there",
                             "lineorder_rows_per_gpu": rows5, "global_lineorder_rows": rows5 * world, "groups": tot_owned[0], "joined_rows": tot_owned[1],
                             "ms": secs5 * 1e3, "rows_per_s": rows5 * world / secs5, "scaling": "weak",
                             "roofline_frac_24B_per_row": 24.0 * rows5 / secs5 / 1e9 / HBM_PEAK_GBS,
                             "exchange_bytes_sent_per_rank": (after["bytes_sent"] - before["bytes_sent"]) // 4,
                             "parity": "35 groups, each owned by exactly one rank; count and profit totals equal to the all-reduced totals of every rank's own "
                                       "one-GPU plan over its rows"}
        del lo, lo_t, dims_dev
    res["transport"] = (f"REHEARSAL, not a measurement: the exchange staged through host memory and gloo, world {world} (ranks may share a GPU)" if rehearsal
                        else f"chgpu_all_to_all_multi / chgpu_all_reduce_u64 over RCCL (C ABI), world {world}")
    comm.close()
    return res


class _HostStagedComm:
    """--backend gloo only: clickhouse_amd.distributed.Comm's surface with every exchange staged through host memory and gloo, so that the
    N>1 orchestration of `sharded_configs` (device partition / merge / join kernels, the ownership and total checks) can be rehearsed with
    several ranks on ONE GPU, where RCCL refuses two ranks on one device.  Its timings mean nothing; the measured transport is D.Comm."""

    def __init__(self, ctx, rank, world, dist, torch, np):
        self.ctx, self.rank, self.world, self.dist, self.torch, self.np = ctx, rank, world, dist, torch, np
        self._sent = self._recv = self._n = 0

    def all_to_all_counts(self, send_counts):
        t = self.torch.tensor([int(x) for x in send_counts], dtype=self.torch.int64)
        r = self.torch.empty_like(t)
        self.dist.all_to_all_single(r, t)
        return [int(x) for x in r.tolist()]

    def all_to_all(self, col, send_counts, recv_counts):
        np, torch = self.np, self.torch
        dt = np.dtype(col.dtype)
        host = col.numpy()
        assert host.shape[0] == sum(send_counts), (host.shape, send_counts)
        snd = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).copy())
        rcv = torch.empty(int(sum(recv_counts)) * dt.itemsize, dtype=torch.uint8)
        self.dist.all_to_all_single(rcv, snd, [int(c) * dt.itemsize for c in recv_counts], [int(c) * dt.itemsize for c in send_counts])
        self._sent += snd.numel()
        self._recv += rcv.numel()
        self._n += 1
        return self.ctx.upload(rcv.numpy().view(dt))

    def all_to_all_multi(self, cols, send_counts):
        recv_counts = self.all_to_all_counts(send_counts)
        return [self.all_to_all(c, send_counts, recv_counts) for c in cols], recv_counts

    def all_reduce_u64(self, values):
        t = self.torch.from_numpy(self.np.array([int(v) % 2**64 for v in values], dtype=self.np.uint64).view(self.np.int64).copy())
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)  # two's complement: the sum mod 2^64
        return [int(x) for x in t.numpy().view(self.np.uint64)]

    def barrier(self):
        self.dist.barrier()

    def stats(self):
        return dict(bytes_sent=self._sent, bytes_received=self._recv, collectives=self._n)

    def close(self):
        pass


def config_q11(args, ctx, ch, torch, np, dev, stream, with_cpu, _headline_cpu):
    """The query shape north_star's target names: SSB Q1.1 -- SELECT sum(lo_extendedprice * lo_discount) WHERE lo_orderdate BETWEEN 19930101 AND
    19931231 AND lo_discount BETWEEN 1 AND 3 AND lo_quantity < 25 -- over the schema's real widths (UInt32 orderdate / extendedprice, UInt8
    discount / quantity: 10 B/row), HBM-resident.  The whole ExpressionActions DAG (five comparisons, four `and`s, one multiply) + FilterTransform
    + sum / count run as ONE generated kernel (chgpu_expr_filter_sum_node); the reference materialises every intermediate column."""
    rows = args.rows
    g = torch.Generator(device=dev).manual_seed(3)
    od = torch.randint(0, 70000, (rows,), dtype=torch.int32, device=dev, generator=g) + 19920101
    disc = torch.randint(0, 11, (rows,), dtype=torch.int32, device=dev, generator=g).to(torch.uint8)
    qty = torch.randint(1, 51, (rows,), dtype=torch.int32, device=dev, generator=g).to(torch.uint8)
    price = torch.randint(90_000, 10_000_000, (rows,), dtype=torch.int32, device=dev, generator=g)
    ts = [od, disc, qty, price]
    cols = [ctx.wrap(t.data_ptr(), np.uint32 if t.dtype == torch.int32 else np.uint8, rows, keepalive=t) for t in ts]
    d = ch.ActionsDAG()
    iod, idisc, iqty, iprice = d.add_input(0, np.uint32), d.add_input(1, np.uint8), d.add_input(2, np.uint8), d.add_input(3, np.uint32)
    c = d.add_column
    f = d.add_function("and", d.add_function("greaterOrEquals", iod, c(19930101, np.uint32)), d.add_function("lessOrEquals", iod, c(19931231, np.uint32)))
    f = d.add_function("and", f, d.add_function("greaterOrEquals", idisc, c(1, np.uint8)))
    f = d.add_function("and", f, d.add_function("lessOrEquals", idisc, c(3, np.uint8)))
    f = d.add_function("and", f, d.add_function("less", iqty, c(25, np.uint8)))
    v = d.add_function("multiply", iprice, idisc)
    ex = d.compile()
    ex.filter_sum(ctx, [c_.cut(0, 4096) for c_ in cols], f, v)   # the first use compiles the kernel (hiprtc): outside the timed region
    dev_ms, wall_ms, (s, cnt) = _timed(lambda: ex.filter_sum(ctx, cols, f, v), torch, stream, reps=10, warmup=2)
    algo = 10.0 * rows
    res = {"workload": "SSB Q1.1-style: sum(lo_extendedprice * lo_discount) under 5 predicates on 3 columns, real column widths (UInt32, UInt8, UInt8, UInt32), "
                       "HBM-resident; the expression DAG + filter + sum as one run-time generated kernel",
           "rows": rows, "selected_rows": int(cnt), "ms": dev_ms, "wall_ms": wall_ms, "rows_per_s": rows / (dev_ms * 1e-3),
           "roofline": {"bound": "hbm", "algorithmic_bytes": algo, "achieved": algo / (dev_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": algo / (dev_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None}}
    if with_cpu:
        import oracle
        oracle.build()
        m = min(rows, 400_000_000)
        host = [t[:m].cpu().numpy().view(np.uint32 if t.dtype == torch.int32 else np.uint8) for t in ts]
        preds = [(0, oracle.GE, 19930101), (0, oracle.LE, 19931231), (1, oracle.GE, 1), (1, oracle.LE, 3), (2, oracle.LT, 25)]
        cores = max(1, len(os.sched_getaffinity(0)))
        bestN = None
        for _ in range(5):
            t0 = time.perf_counter()
            rN = oracle.expr_filter_sum_pipeline(host, preds, oracle.VAL_MUL, 3, 1, threads=cores)
            dt = time.perf_counter() - t0
            bestN = dt if bestN is None else min(bestN, dt)
        m1 = min(m, 50_000_000)
        t0 = time.perf_counter()
        oracle.expr_filter_sum_pipeline([h[:m1] for h in host], preds, oracle.VAL_MUL, 3, 1, threads=1)
        t1 = time.perf_counter() - t0
        sg, cg = ex.filter_sum(ctx, [c_.cut(0, m) for c_ in cols], f, v)
        assert (int(sg), int(cg)) == (int(rN[0]), int(rN[1])), "Q11: GPU differs from the CPU restatement"
        res["cpu_baseline"] = {"value": m / bestN, "unit": "rows/s", "cores": cores, "kind": "port",
                               "sample": f"first {m} rows, Blocks of 65409 rows, per Block: five comparisons -> UInt8 masks, four `and`s, the product column, "
                                         f"IColumn::filter, sum (the reference's one-function-per-action execution), best of 5 on {cores} threads; "
                                         f"single thread over {m1} rows: {m1 / t1:.4g} rows/s",
                               "single_thread_value": m1 / t1}
        res["gpu_over_cpu_all_cores"] = rows / (dev_ms * 1e-3) / (m / bestN)
        res["parity"] = "sum and count bit-exact on the sample"
    return res


def config_c2_from_host_blocks(args, ctx, ch, torch, np, dev, stream, with_cpu, headline_cpu):
    """The honest end-to-end of configs[1]: the Int64 rows START IN HOST MEMORY as Blocks of 65 409 rows.  The C++ shim (host/pipeline_demo
    --bench-host-blocks) runs `streams` pipeline threads, each gluing its Blocks into pinned stripes (StripeBuilder), uploading them asynchronously
    and running the fused filter + sum per stripe: rows/s INCLUDING the upload -- bounded by the host link, never the `value`."""
    import subprocess
    exe = os.path.join(REPO, "clickhouse_amd", "host", "pipeline_demo")
    rows = min(args.rows, 400_000_000)
    best = None
    for streams in (4, 8):
        p = subprocess.run([exe, "--bench-host-blocks", str(rows), str(streams), str(2 << 20)], capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError(f"pipeline_demo --bench-host-blocks failed: {p.stderr[-300:]}")
        r = json.loads(p.stdout.strip().splitlines()[-1])
        if best is None or r["rows_per_s_pcie_inclusive"] > best["rows_per_s_pcie_inclusive"]:
            best = r
    res = {"workload": "configs[1] fed from HOST Blocks of 65409 Int64 rows: pinned stripes (StripeBuilder), asynchronous uploads overlapped with the fused "
                       "filter + sum of the previous stripe, several pipeline streams (C++ shim, host/pipeline_demo --bench-host-blocks); PCIe-inclusive",
           "rows": rows, "streams": best["streams"], "stripe_rows": best["stripe_rows"], "rows_per_s": best["rows_per_s_pcie_inclusive"],
           "host_link_GBps": best["host_GBps"], "parity": "sum and count equal to the host's own loop over the same rows (checked inside the run)"}
    if headline_cpu:
        res["cpu_all_cores_rows_per_s"] = headline_cpu["value"]
        res["vs_cpu_all_cores"] = best["rows_per_s_pcie_inclusive"] / headline_cpu["value"]
        res["crossover"] = ("data that starts in host memory moves at the host link's rate: the GPU path wins only against fewer than about "
                            f"{best['rows_per_s_pcie_inclusive'] / headline_cpu['single_thread_value']:.0f} CPU threads of this box for this one-pass query; "
                            "the >= 10x target holds for HBM-resident stripes (the headline) and for plans that reuse uploaded columns")
    return res


def _timed(fn, torch, stream, reps, warmup=1):
    """fn() launches on `stream`; -> (mean device ms between HIP events on that stream, mean wall ms incl. the host synchronisation, last result)"""
    r = None
    for _ in range(warmup):
        r = fn()
    stream.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(e0.elapsed_time(e1))
    return sum(dev_ms) / len(dev_ms), sum(wall_ms) / len(wall_ms), r


def _kernels_from_profile(prefixes):
    """per-kernel average ms of the committed rocprofv3 --kernel-trace --stats summary of this command (profiles/): the live number in
    the line is the HIP-event bracket around the whole operator; this list says how it splits"""
    import csv
    import glob
    paths = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_bench_kernel_stats.csv")))
    if not paths:
        return None, None
    rows = []
    with open(paths[-1]) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            short = name[5:] if name.startswith("void ") else name
            if any(short.startswith(p) for p in prefixes if "<" not in p) or any(all(t in short for t in p.split("<")) for p in prefixes if "<" in p):
                rows.append({"kernel": name[:96], "calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) / 1e6})
    return rows, os.path.relpath(paths[-1], REPO)


def config_c3(args, ctx, ch, torch, np, dev, stream, tj, with_cpu):
    """BASELINE.json configs[2]: SELECT k, sum(v), count() GROUP BY k -- UInt32 key uniform in [0, 1e6), Int64 values, 1e9 rows resident
    in HBM, size hint given (the reference passes statistics-based hints too: Aggregator.cpp:107-128).  One operator call =
    chgpu_agg_create + chgpu_agg_add_block over the whole stripe (table creation and the control-block read-back included)."""
    rows = args.c3_rows
    g = torch.Generator(device=dev).manual_seed(2)
    k = torch.randint(0, 1_000_000, (rows,), dtype=torch.int32, device=dev, generator=g)
    v = torch.randint(-2**31, 2**31, (rows,), dtype=torch.int64, device=dev, generator=g)
    kc = ctx.wrap(k.data_ptr(), np.uint32, rows, keepalive=k)
    vc = ctx.wrap(v.data_ptr(), np.int64, rows, keepalive=v)
    aggs = [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)]

    def run(n=rows):
        A = ch.Aggregator(np.uint32, aggs, size_hint=1_000_000, ctx=ctx)
        A.execute_on_block(kc, [vc, None], 0, n)
        return A

    dev_ms, wall_ms, A = _timed(run, torch, stream, reps=5, warmup=2)
    groups = len(A)
    # size-independent check at full size: every key once, counts partition the rows, sum of sums == sum of the column (mod 2^64)
    gk, (gs, gc) = A.convert_to_block()
    assert np.unique(gk).shape[0] == gk.shape[0] == groups and int(gc.sum()) == rows
    assert int(gs.astype(np.uint64).sum()) == int(v.sum().item()) % 2**64
    algo = 12.0 * rows  # 4 B key + 8 B value per row
    kernels, ksrc = _kernels_from_profile(["k_gb_", "k_agg_", "k_tile_", "k_rp_<GbpPartFn"])
    res = {"workload": "GROUP BY UInt32 key (1 M groups), sum(Int64) + count(), HBM-resident, size_hint=1e6",
           "rows": rows, "groups": groups, "calls": 7, "ms": dev_ms, "wall_ms": wall_ms, "rows_per_s": rows / (dev_ms * 1e-3),
           "roofline": {"bound": "hbm", "algorithmic_bytes": algo, "achieved": algo / (dev_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": algo / (dev_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": tj.get("C3_hbm_bytes_per_call"),
                        "traffic_source": tj.get("source") if tj.get("C3_hbm_bytes_per_call") else None,
                        "kernels": kernels, "kernels_source": ksrc}}
    if with_cpu:
        import oracle
        oracle.build()
        avail = max(1, len(os.sched_getaffinity(0)))
        sample = min(rows, 400_000_000)
        # One AggregatedDataVariants per stream: every stream builds its own table of (nearly) all groups before it reaches the steady
        # state this config is about, so streams only pay while rows per stream >> groups -- as in the reference, where max_threads
        # streams share 1e9 rows.  On a bounded sample that means fewer streams, not fewer rows per stream: >= 16 rows per group and stream.
        cores = max(1, min(avail, sample // (16 * 1_000_000)))
        ks = k[:sample].cpu().numpy().view(np.uint32)
        vs = v[:sample].cpu().numpy()
        t0 = time.perf_counter()
        ref, secs = oracle.groupby_pipeline(ks, aggs, [vs, None], threads=cores)
        tN = time.perf_counter() - t0
        all_note = ""
        if avail > cores:  # and with every core, for the record: the better of the two is the baseline
            t0 = time.perf_counter()
            ref_all, secs_all = oracle.groupby_pipeline(ks, aggs, [vs, None], threads=min(avail, 256))
            t_all = time.perf_counter() - t0
            all_note = f"; with all {min(avail, 256)} cores as streams: {sample / t_all:.4g} rows/s"
            if t_all < tN:
                ref, secs, tN, cores, all_note = ref_all, secs_all, t_all, min(avail, 256), f"; with {cores} streams: {sample / tN:.4g} rows/s"
            del ref_all
        s1 = min(sample, 40_000_000)
        t0 = time.perf_counter()
        oracle.groupby_pipeline(ks[:s1], aggs, [vs[:s1], None], threads=1)
        t1 = time.perf_counter() - t0
        # parity on the sample: keys, sums and counts bit for bit
        ok, (os_, oc) = ref.convert_to_block()
        sk, (ss, sc) = run(sample).convert_to_block()
        i, j = np.argsort(sk), np.argsort(ok)
        assert np.array_equal(sk[i], ok[j]) and np.array_equal(ss[i], os_[j]) and np.array_equal(sc[i], oc[j]), "C3: GPU differs from the CPU restatement"
        res["cpu_baseline"] = {"value": sample / tN, "unit": "rows/s", "cores": cores, "kind": "port",
                               "sample": f"first {sample} rows, Blocks of 65409 rows, {cores} of {avail} available cores as streams (>= 16 rows per group and "
                                         f"stream: more streams only build more 1 M-group tables on a bounded sample), each with its own table and the "
                                         f"reference's hash-cell prefetch, two-level bucket-parallel merge ({secs[0]:.2f} s consume + {secs[1]:.2f} s merge); "
                                         f"single stream over {s1} rows: {s1 / t1:.4g} rows/s{all_note}",
                               "single_thread_value": s1 / t1}
        res["parity"] = "bit-exact on the sample (keys, sums, counts) + full-size partition properties"
    return res


def config_c4(args, ctx, ch, torch, np, dev, stream, tj, with_cpu):
    """BASELINE.json configs[3], the share of ONE GPU: 1e8-row probe INNER JOIN 1e7-row build on a UInt64 key (unique build keys, ~50 %
    hits), checksum form SELECT count(), sum(bv).  build = chgpu_join_create + add_block + finish_build; probe = the join with the
    aggregation fused behind it.  The hash table is lazy (built by the first joinBlock / key-count consumer): this fused probe joins
    without one -- every timed probe call partitions the build rows and the probe keys and builds + probes the slices in LDS -- so the
    build phase is the key staging alone and the whole cost of the join sits in probe_ms."""
    nb, npb = args.c4_build_rows, args.c4_probe_rows
    g = torch.Generator(device=dev).manual_seed(5)
    bk = (torch.randperm(nb, device=dev, generator=g).to(torch.int64) + 1) * 2654435761
    pk = torch.where(torch.rand(npb, device=dev, generator=g) < 0.5, bk[torch.randint(0, nb, (npb,), device=dev, generator=g)],
                     torch.randint(0, 2**62, (npb,), dtype=torch.int64, device=dev, generator=g))
    bv = torch.randint(-2**40, 2**40, (nb,), dtype=torch.int64, device=dev, generator=g)
    bkc = ctx.wrap(bk.data_ptr(), np.uint64, nb, keepalive=bk)
    pkc = ctx.wrap(pk.data_ptr(), np.uint64, npb, keepalive=pk)
    bvc = ctx.wrap(bv.data_ptr(), np.int64, nb, keepalive=bv)

    def build():
        j = ch.HashJoin(ch.JOIN_INNER, ch.STRICT_ALL, ctx=ctx)
        j.add_block(bkc)
        j.finish_build()
        return j

    def probe(j, pcol):
        return j.probe_count_sum(pcol, bvc)  # (count, sum bits)

    # two warm-up builds: a join table lives in the context's column pool, and with one build alive while the next is made the pool
    # cycles two blocks -- the timed builds then reuse them (the steady state of a pipeline; a cold hipMalloc of 1.5 GB costs ~30 ms)
    b_reps, b_warm, p_reps, p_warm = 3, 2, 5, 3
    b_ms, b_wall, j = _timed(build, torch, stream, reps=b_reps, warmup=b_warm)
    p_ms, p_wall, (cnt, sm) = _timed(lambda: probe(j, pkc), torch, stream, reps=p_reps, warmup=p_warm)
    # independent check at full size: membership by a sorted-array search, payload through the same permutation
    sbk, order = torch.sort(bk)
    pos = torch.searchsorted(sbk, pk).clamp_(max=nb - 1)
    hit = sbk[pos] == pk
    want_cnt = int(hit.sum().item())
    want_sum = int(bv[order[pos[hit]]].sum().item()) % 2**64
    assert (cnt, sm % 2**64) == (want_cnt, want_sum), ("C4", cnt, sm, want_cnt, want_sum)
    del sbk, order, pos, hit
    algo = 8.0 * npb + 16.0 * nb + 8.0 * cnt  # probe keys + build keys and payload + payload per matched row
    kernels, ksrc = _kernels_from_profile(["k_join_", "k_jp_", "k_rp_<JoinRegionFn", "k_rp_<JoinBucket2Fn", "k_rp_<JoinSliceFn", "k_rp_<JoinRadixFn"])
    tot = b_ms + p_ms
    res = {"workload": "100 M-row probe INNER JOIN 10 M-row build on UInt64 (ALL, unique build keys, ~50 % hits), SELECT count(), sum(bv); one GPU",
           "plan": "radix join: build rows {key, payload} and probe keys partitioned twice down to 4096-cell slices, every slice built and probed in LDS; "
                   "no hash table in HBM (it is lazy: joinBlock / key-count consumers build it), so build_ms is key staging and probe_ms the whole join",
           "build_rows": nb, "probe_rows": npb, "matches": cnt, "build_calls": b_reps + b_warm, "probe_calls": p_reps + p_warm, "build_ms": b_ms, "probe_ms": p_ms, "ms": tot, "wall_ms": b_wall + p_wall,
           "rows_per_s": (nb + npb) / (tot * 1e-3), "probe_rows_per_s": npb / (p_ms * 1e-3),
           "roofline": {"bound": "hbm", "algorithmic_bytes": algo, "achieved": algo / (tot * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": algo / (tot * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": tj.get("C4_hbm_bytes_per_call"),
                        "traffic_source": tj.get("source") if tj.get("C4_hbm_bytes_per_call") else None,
                        "kernels": kernels, "kernels_source": ksrc}}
    if with_cpu:
        import oracle
        oracle.build()
        cores = max(1, len(os.sched_getaffinity(0)))
        bk_h, bv_h = bk.cpu().numpy().view(np.uint64), bv.cpu().numpy()
        pk_h = pk.cpu().numpy().view(np.uint64)
        c_cnt, c_sum, t_b, t_p = oracle.join_count_sum_pipeline(bk_h, bv_h, pk_h, threads=cores)
        assert (c_cnt, c_sum) == (cnt, sm % 2**64), "C4: GPU differs from the CPU restatement"
        s1 = min(npb, 20_000_000)
        _, _, _, t_p1 = oracle.join_count_sum_pipeline(bk_h, bv_h, pk_h[:s1], threads=1)
        res["cpu_baseline"] = {"value": (nb + npb) / (t_b + t_p), "unit": "rows/s", "cores": cores, "kind": "port",
                               "sample": f"the whole config: build by one stream ({nb / t_b:.4g} rows/s), probe + payload gather + sum by {cores} streams over "
                                         f"Blocks of 65409 rows ({npb / t_p:.4g} rows/s); single probe stream over {s1} rows: {s1 / t_p1:.4g} rows/s",
                               "build_rows_per_s": nb / t_b, "probe_rows_per_s": npb / t_p, "single_thread_probe_value": s1 / t_p1}
        res["parity"] = "count and sum(payload) bit-exact against the CPU restatement and an independent sorted-search join, full size"
    return res


def config_c5(args, ctx, ch, torch, np, dev, stream, with_cpu):
    """BASELINE.json configs[4], the share of ONE GPU of the 6 B-row lineorder table (750 M rows at 8 GPUs; customer 30 M, supplier 2 M,
    part 2 M rows replicated and HBM-resident): SSB Q4.1-style plan -- dimension filters, two semi joins, two inner joins with payload,
    GROUP BY (year, nation) with packed keys, sum(revenue) - sum(supplycost) -- composed from the hot-path operators (tools/ssb.py)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import ssb
    rows = args.c5_rows
    C, S, P = 30_000_000, 2_000_000, 2_000_000
    dims = ssb.gen_dims(C, S, P)
    lo_t = ssb.gen_lineorder_torch(rows, C, S, P, dev)
    lo = {k: ctx.wrap(v.data_ptr(), np.uint32, rows, keepalive=v) for k, v in lo_t.items()}
    dims_dev = ssb.upload_dims(ctx, dims)
    dev_ms, wall_ms, res = _timed(lambda: ssb.q41_gpu(ch, ctx, dims_dev, lo), torch, stream, reps=5, warmup=3)
    algo = 24.0 * rows  # six 4-byte lineorder columns
    out = {"workload": "SSB Q4.1-style: 2 semi joins + 2 inner joins with payload + GROUP BY (year, nation), sum(revenue) - sum(supplycost); one GPU's share "
                       "of the 6 B-row lineorder table, dimension columns resident in HBM (their filters and the four hash-table builds inside the timed plan)",
           "lineorder_rows": rows, "groups": len(res), "ms": wall_ms, "device_ms": dev_ms, "rows_per_s": rows / (wall_ms * 1e-3),
           "roofline": {"bound": "hbm", "algorithmic_bytes": algo, "achieved": algo / (wall_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": algo / (wall_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None}}
    try:  # the last committed PMC collection of the plan on its own (tools/gpu_pmc_c5.sh), quoted only for the same workload
        ts = json.load(open(os.path.join(REPO, "profiles", "traffic_ssb.json")))
        if ts.get("algorithmic_bytes") == algo:
            out["roofline"]["traffic"] = ts.get("C5_hbm_bytes_per_run")
            out["roofline"]["traffic_source"] = (f"profiles/{ts.get('tag', '')}_traffic_ssb.json (= profiles/traffic_ssb.json): rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE "
                                                 "passes of `bench.py --full --only-c5`, tools/gpu_pmc_c5.sh")
    except Exception:
        pass
    if with_cpu:
        import oracle
        oracle.build()
        threads = max(1, min(32, len(os.sched_getaffinity(0))))  # streams beyond this only contend for the interpreter lock of the per-Block driver
        m = min(rows, 60_000_000)
        lo_s = {k: v[:m].cpu().numpy().view(np.uint32) for k, v in lo_t.items()}
        t0 = time.perf_counter()
        want = ssb.q41_cpu(oracle, dims, lo_s, threads=threads)
        t_cpu = time.perf_counter() - t0
        got = ssb.q41_gpu(ch, ctx, dims_dev, {k: c.cut(0, m) for k, c in lo.items()})
        assert got == want, "C5: the GPU plan differs from the CPU restatement on the sample"
        out["cpu_baseline"] = {"value": m / t_cpu, "unit": "rows/s", "cores": threads, "kind": "port",
                               "sample": f"first {m} lineorder rows through the same plan over the oracle, Blocks of 65409 rows, {threads} streams sharing the four "
                                         "right-side tables, own aggregation states merged at the end (dimension filters and builds included)"}
        out["parity"] = "every (year, nation) group: profit and row count bit-exact on the sample"
    return out


def dump_outputs(out_dir, state, np):
    """--dump-outputs: what a caller of the timed path receives, sum(a) (Int64) and count(), as float64 arrays.  A float64 holds
    integers exactly only up to 2^53 and the sum of 1 B rows passes that, so sum_words.npy adds the sum's two's-complement bits as
    two exact 32-bit halves {high, low}."""
    os.makedirs(out_dir, exist_ok=True)
    s, c = int(state[0]), int(state[1])
    bits = s % 2**64
    np.save(os.path.join(out_dir, "sum.npy"), np.array([s], dtype=np.float64))
    np.save(os.path.join(out_dir, "count.npy"), np.array([c], dtype=np.float64))
    np.save(os.path.join(out_dir, "sum_words.npy"), np.array([bits >> 32, bits & 0xFFFFFFFF], dtype=np.float64))


def cpu_baseline(a, sample_rows, ctx, ch):
    """The reference CPU path restated (oracle/, kind 'port') timed on this box's host cores over a bounded sample of the
    same column: per-Block (65 409 rows) compare -> UInt8 mask -> countBytesInFilter -> IColumn::filter -> sum addMany.
    The oracle is only the thing timed/compared here, never part of the GPU path."""
    import numpy as np

    import oracle

    oracle.build()
    m = min(sample_rows, a.shape[0])
    host = a[:m].cpu().numpy()
    cores = max(1, len(os.sched_getaffinity(0)))  # every core this process may run on
    best1, bestN = None, None
    r1 = rN = None
    for _ in range(5):
        t0 = time.perf_counter()
        r1 = oracle.filter_sum_pipeline(host, oracle.LT, THRESHOLD, threads=1)
        dt = time.perf_counter() - t0
        best1 = dt if best1 is None else min(best1, dt)
    for _ in range(20):
        t0 = time.perf_counter()
        rN = oracle.filter_sum_pipeline(host, oracle.LT, THRESHOLD, threads=cores)
        dt = time.perf_counter() - t0
        bestN = dt if bestN is None else min(bestN, dt)
    # parity on the sample: the HIP path must give the CPU path's answer bit for bit
    s, c = ch.filter_sum(ctx.wrap(a.data_ptr(), np.int64, m, keepalive=a), ch.LT, THRESHOLD)
    assert (int(s), c) == (int(r1[0]), r1[1]) == (int(rN[0]), rN[1]), "GPU result differs from the CPU restatement"
    return {
        "value": m / bestN,
        "unit": "rows/s",
        "cores": cores,
        "kind": "port",
        "sample": f"first {m} rows of the same column, Blocks of 65409 rows, best of 20 ({cores} threads) ; "
                  f"single thread: {m / best1:.4g} rows/s (best of 5); about 7 s of CPU work in all",
        "single_thread_value": m / best1,
    }


if __name__ == "__main__":
    main()
