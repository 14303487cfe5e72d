#!/usr/bin/env python3
"""bench.py — TPC-H Q1 scan/filter/agg benchmark (BASELINE.json metric:
rows/sec + achieved HBM GB/s on TPC-H Q1, SF100 per GPU).

A "step" = one full pass of the fused Q1 path over this rank's HBM-resident
lineitem columns (device-generated TPC-H data, 38 B/row algorithmic). N>1 =
one process per GPU over RCCL (weak scaling: SF100 shard per GPU = one part of
SF 100*N), plus the partial-state exchange leg (BASELINE config 4 shape).

Run:  python bench.py [--gpus N] [--steps K] [--warmup W] [--sf-per-gpu S]
                       [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints one JSON result
line. --full adds the legs that take runs of their own (the CPU baseline).
--dump-outputs DIR writes what the last timed step returned as DIR/<name>.npy.
Driver launches N>1 via torch.distributed.run; reads RANK/WORLD_SIZE/etc.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK_GBPS = 8000.0         # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
ALG_BYTES_PER_ROW = 38         # shipdate i32 + 4*f64 + 2*u8
Q1_CUTOFF = 10471              # 1998-09-02 (shipdate <= date '1998-12-01' - 90 day)


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(msg, file=sys.stderr, flush=True)


def merge_raw(raws):
    """Exact cross-rank merge of raw integer Q1 accumulators (python ints)."""
    total = [0] * 60
    for raw in raws:
        for c in range(6):
            for f in range(4):  # u128 fields
                lo, hi = raw[c * 10 + 2 * f], raw[c * 10 + 2 * f + 1]
                cur = total[c * 10 + 2 * f] | (total[c * 10 + 2 * f + 1] << 64)
                cur += lo | (hi << 64)
                total[c * 10 + 2 * f] = cur & ((1 << 64) - 1)
                total[c * 10 + 2 * f + 1] = cur >> 64
            total[c * 10 + 8] += raw[c * 10 + 8]
            total[c * 10 + 9] += raw[c * 10 + 9]
    return total


def exchange_partials(tdist, world, rank, raw_u64, device):
    """Exchange leg of BASELINE config 4: route each group's partial state to
    its owner rank (PagePartitioner-equivalent assignment over the group key,
    see combo_owner_rank) with an all_to_all over RCCL; on gloo (CPU tests,
    which lacks alltoall) the same routing runs over all_gather + local
    selection — identical results, different transport. Returns the exact
    integer merge of the states this rank owns (python big-ints)."""
    import torch
    signed = [x - (1 << 64) if x >= (1 << 63) else x for x in raw_u64]
    raw = torch.tensor(signed, dtype=torch.int64, device=device).view(6, 10)
    send = [torch.zeros(6, 10, dtype=torch.int64, device=device) for _ in range(world)]
    for c in range(6):
        send[combo_owner_rank(c, world)][c] = raw[c]
    if tdist.get_backend() == "nccl":
        recv = [torch.empty(6, 10, dtype=torch.int64, device=device) for _ in range(world)]
        tdist.all_to_all(recv, send)
    else:
        stacked = torch.stack(send)                       # [world][6][10]
        allv = [torch.empty_like(stacked) for _ in range(world)]
        tdist.all_gather(allv, stacked)
        recv = [allv[r][rank] for r in range(world)]
    return merge_raw([[x & ((1 << 64) - 1) for x in t.flatten().tolist()] for t in recv])


def combo_owner_rank(combo, world):
    """Exchange routing for the partial->final aggregation leg: the canonical
    row hash of the (returnflag, linestatus) group key (31*combine of the
    bigint xxmix per channel — HashGenerator.java:20, AbstractLongType.java:
    121-125) reduced by the remote partition function (HashGenerator.java:
    41-46)."""
    m = (1 << 64) - 1

    def rotl(x, r):
        return ((x << r) | (x >> (64 - r))) & m

    def xxmix(v):
        return (rotl((v * 0xC2B2AE3D27D4EB4F) & m, 31) * 0x9E3779B185EBCA87) & m

    rf, ls = combo // 2, combo % 2
    h = (31 * xxmix(rf) + xxmix(ls)) & m
    lh = (h ^ (h >> 32)) & 0xFFFFFFFF
    return (lh * world) >> 32


Q1_F64_FIELDS = ("sum_qty", "sum_base", "sum_disc_price", "sum_charge",
                 "avg_qty", "avg_price", "avg_disc", "sum_disc")


def _u64_words(vals):
    """u64 accumulator words as an [n, 2] float64 array of (low, high) 32-bit
    halves: every value is exact in float64."""
    import numpy as np
    return np.array([[v & 0xFFFFFFFF, v >> 32] for v in vals], dtype=np.float64)


def dump_q1_outputs(dirpath, res, merged=None):
    """Write the Q1Result a caller of the timed path receives (and, at N>1,
    this rank's merged exchange state) as DIR/<name>.npy, float64."""
    import numpy as np
    os.makedirs(dirpath, exist_ok=True)
    for f in Q1_F64_FIELDS:
        np.save(os.path.join(dirpath, f + ".npy"),
                np.array(list(getattr(res, f)), dtype=np.float64))
    np.save(os.path.join(dirpath, "count.npy"),
            np.array(list(res.count), dtype=np.float64))
    np.save(os.path.join(dirpath, "raw.npy"), _u64_words(list(res.raw)))
    if merged is not None:
        np.save(os.path.join(dirpath, "merged_raw.npy"), _u64_words(merged))


def main():
    # this libomp's first parallel region costs ~2.5 s when OMP_NUM_THREADS
    # is unset (measured; 0.4 s with it set) — pin the default before the
    # parquet decode / cpu_baseline legs initialize the runtime. Explicit
    # omp_set_num_threads calls (the calibrated baseline) still override.
    os.environ.setdefault("OMP_NUM_THREADS", str(os.cpu_count() or 8))
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sf-per-gpu", type=float, default=100.0)
    ap.add_argument("--workload", choices=["q1", "q3", "sweep", "parquet"],
                    default="q1")
    ap.add_argument("--skip-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beyond the headline figure "
                         "(the host-core CPU baseline of the q1 workload)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step returned as DIR/<name>.npy (float64)")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="gloo only for multi-rank validation on one GPU "
                         "(RCCL requires distinct devices per rank)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    if args.dump_outputs and args.workload == "sweep":
        ap.error("--dump-outputs is not available for --workload sweep")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    n_gpus = max(world, args.gpus)

    import torch
    dist = None
    if world > 1:
        import torch.distributed as tdist
        dist = tdist
        # modulo: lets world_size-2 validation runs share a 1-GPU box
        local_rank = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local_rank)
        tdist.init_process_group(backend=args.backend)

    import trino_amd

    sess = trino_amd.Session(local_rank)

    if args.workload == "q3":
        run_q3(args, sess, n_gpus, rank, dist)
        sess.close()
        if dist:
            dist.destroy_process_group()
        return
    if args.workload == "sweep":
        run_sweep(args, sess, n_gpus, rank)
        sess.close()
        if dist:
            dist.destroy_process_group()
        return
    if args.workload == "parquet":
        run_parquet(args, sess, n_gpus, rank)
        sess.close()
        if dist:
            dist.destroy_process_group()
        return

    # ---- workload: this rank's shard of SF (sf_per_gpu * N): contiguous
    # order parts, exactly TpchSplit(part, totalParts) semantics ----
    total_sf = args.sf_per_gpu * n_gpus
    total_orders = int(1_500_000 * args.sf_per_gpu) * n_gpus
    per = total_orders // n_gpus
    order_start = 1 + rank * per
    order_count = per + (total_orders % n_gpus if rank == n_gpus - 1 else 0)

    t0 = time.time()
    cols = sess.tpch_lineitem(total_sf, order_start, order_count)
    rows_rank = cols.row_count
    log(f"generated {rows_rank:,} lineitem rows/rank (SF{total_sf:g} part {rank+1}/{n_gpus}) "
        f"in {time.time()-t0:.1f}s — {rows_rank*ALG_BYTES_PER_ROW/2**30:.1f} GiB in HBM")

    coll_dev = "cuda" if (dist and dist.get_backend() == "nccl") else "cpu"
    if dist:
        rows_t = torch.tensor([rows_rank], dtype=torch.int64, device=coll_dev)
        dist.all_reduce(rows_t)
        rows_total = int(rows_t.item())
    else:
        rows_total = rows_rank

    def step():
        r = sess.q1(cols, Q1_CUTOFF)
        if dist:
            # exchange leg (config 4 shape): partial->exchange->final agg
            merged = exchange_partials(dist, world, rank, list(r.raw), coll_dev)
            return r, merged
        return r, None

    # warmup
    for _ in range(args.warmup):
        res, _ = step()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()

    kernel_ms = []
    t_start = time.time()
    for _ in range(args.steps):
        res, merged = step()
        kernel_ms.append(res.elapsed_ms)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.time() - t_start
    if dist:
        el = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        elapsed = float(el.item())

    ms_per_step = elapsed * 1000.0 / args.steps
    value = rows_total / (elapsed / args.steps)          # whole-job rows/s
    k_ms = sum(kernel_ms) / len(kernel_ms)
    achieved_gbps = rows_rank * ALG_BYTES_PER_ROW / (k_ms / 1000.0) / 1e9

    if args.dump_outputs and rank == 0:
        dump_q1_outputs(args.dump_outputs, res, merged)

    # ---- CPU baseline (--full; rank 0, N=1 only): the parity-pinned oracle
    # timed on host cores over a bounded sample (SF1 = 6,001,215 rows,
    # repeated) ----
    cpu_baseline = None
    if args.full and rank == 0 and n_gpus == 1 and not args.skip_cpu_baseline:
        import oracle
        cores = os.cpu_count() or 1
        li = oracle.gen_lineitem(1.0)
        n_s = len(li["shipdate"])
        # calibrate the OpenMP thread count (oversubscription on many-core
        # hosts collapses throughput on this cache-resident sample)
        best_t, best_rate = 1, 0.0
        for t in sorted({1, 8, 16, 32, min(64, cores), cores}):
            t0 = time.time()
            oracle.q1_exact(li, Q1_CUTOFF, threads=t)
            oracle.q1_exact(li, Q1_CUTOFF, threads=t)
            rate = 2 * n_s / (time.time() - t0)
            if rate > best_rate:
                best_t, best_rate = t, rate
        reps, spent = 0, 0.0
        tcb = time.time()
        while spent < 10.0 and reps < 500:
            oracle.q1_exact(li, Q1_CUTOFF, threads=best_t)
            reps += 1
            spent = time.time() - tcb
        cpu_rows_s = n_s * reps / spent
        cpu_baseline = {
            "value": cpu_rows_s, "unit": "rows/s", "cores": best_t, "kind": "port",
            "sample": f"TPC-H SF1 lineitem ({n_s:,} rows) x{reps} passes, "
                      f"{spent:.1f}s, OpenMP {best_t} threads (calibrated over "
                      f"{{1..{cores}}}); generator excluded",
        }
        log(f"cpu_baseline: {cpu_rows_s/1e6:.0f} Mrow/s on {best_t} threads")

    if rank == 0:
        out = {
            "metric": "tpch_q1_scan_filter_agg_throughput",
            "value": value,
            "unit": "rows/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,   # reference publishes no numbers
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": f"TPC-H Q1 (lineitem scan+filter+agg) SF{args.sf_per_gpu:g}"
                            f" per GPU, HBM-resident device-generated columns",
                "scale_factor_total": total_sf,
                "rows_total": rows_total,
                "parallelism": f"dp{n_gpus}",
                "cutoff": "shipdate <= 1998-09-02",
            },
            "roofline": {
                "bound": "hbm",
                "achieved": achieved_gbps,
                "peak": HBM_PEAK_GBPS,
                "unit": "GB/s",
                "frac": achieved_gbps / HBM_PEAK_GBPS,
                "traffic": None,   # PMC evidence: profiles/ (separate rocprofv3 --pmc runs)
            },
            "cpu_baseline": cpu_baseline,
        }
        print(json.dumps(out), flush=True)

    sess.tpch_lineitem_free(cols)
    sess.close()
    if dist:
        dist.destroy_process_group()


def run_q3(args, sess, n_gpus, rank, tdist=None):
    """BASELINE config 3: TPC-H Q3 3-way join build/probe.
    Timed region = the full operator pipeline (2 joins + agg + topn) over
    HBM-resident inputs; metric = probe-side lineitem rows per second
    (whole-job aggregate over ranks).

    N>1 (weak scaling, SF = sf_per_gpu x N): rank r generates customer/
    orders/lineitem for ITS contiguous key ranges; orders⨝lineitem is
    co-partitioned by construction; the small filtered-customer build is
    BROADCAST (all_gather union — trino_amd/dist.py) inside the timed
    region, like the reference's replicated join; per-rank TopNs merge at
    the end (orderkey ranges are rank-disjoint)."""
    import torch
    from trino_amd import tpch_queries
    from trino_amd import dist as tgdist
    world = tdist.get_world_size() if tdist else 1
    sf = args.sf_per_gpu
    order_count = int(1_500_000 * sf)
    cust_count = int(150_000 * sf)
    t0 = time.time()
    inp = tpch_queries.q3_prepare(
        sess, sf * world,
        order_start=rank * order_count + 1, order_count=order_count,
        cust_start=rank * cust_count + 1, cust_count=cust_count)
    rows = inp["li"].row_count
    log(f"q3 inputs ready: {rows:,} lineitem rows/rank, SF{sf * world:g} "
        f"({world} ranks), {time.time()-t0:.1f}s")
    hook = None
    if world > 1 and args.backend == "nccl":
        import ctypes as _ct
        from trino_amd import _lib as _tglib
        _tglib.tg_copy_dtod.restype = _ct.c_int
        _tglib.tg_copy_dtod.argtypes = [_ct.c_void_p] * 3 + [_ct.c_int64]

        def hook(session, dev_page):
            n = dev_page.position_count
            t = torch.empty(max(int(n), 1), dtype=torch.int64, device="cuda")
            if n:
                _tglib.tg_copy_dtod(session._h, t.data_ptr(),
                                    dev_page.blocks[0].data, int(n) * 8)
            return tgdist.gather_union_device(tdist, t[:int(n)])
        hook.device_resident = True
    elif world > 1:
        hook = lambda keys: tgdist.gather_union(tdist, keys)
    for _ in range(args.warmup):
        tpch_queries.q3_execute(sess, inp, download_groups=False,
                                cust_key_exchange=hook)
    torch.cuda.synchronize()
    if tdist:
        tdist.barrier()
    t_start = time.time()
    for _ in range(args.steps):
        r = tpch_queries.q3_execute(sess, inp, download_groups=False,
                                    cust_key_exchange=hook)
    torch.cuda.synchronize()
    elapsed = time.time() - t_start
    if tdist:
        dev = "cuda" if tdist.get_backend() == "nccl" else "cpu"
        t_el = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        tdist.all_reduce(t_el, op=tdist.ReduceOp.MAX)
        elapsed = float(t_el.item())           # max over ranks
        t_rows = torch.tensor([rows], dtype=torch.float64, device=dev)
        tdist.all_reduce(t_rows, op=tdist.ReduceOp.SUM)
        rows = int(t_rows.item())              # whole-job rows
        r["top10"] = tgdist.merge_topn(tdist, r["top10"], 10,
                                       key=lambda t: (-t[1], t[2]))
    tpch_queries.q3_release(sess, inp)
    if args.dump_outputs and rank == 0:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "top10.npy"),
                np.array(r["top10"], dtype=np.float64).reshape(-1, 4))
    ms = elapsed * 1000 / args.steps
    value = rows / (elapsed / args.steps)
    out = {
        "metric": "tpch_q3_join_probe_throughput",
        "value": value, "unit": "rows/s", "n_gpus": n_gpus,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"TPC-H Q3 (3-way hash join build/probe) "
                               f"SF{sf * (tdist.get_world_size() if tdist else 1):g} "
                               f"on {n_gpus}xMI355X",
                   "rows_lineitem": rows, "parallelism": f"dp{n_gpus}",
                   "top10_first": r["top10"][0] if r["top10"] else None},
        "roofline": {
            "bound": "hbm",
            # dominant kernel = the orderkey probe (count+fill passes), HIP
            # event-timed per step inside q3_execute. Algorithmic bytes =
            # count pass 8 B/probe row + fill pass 16 B/probe row read +
            # 16 B/match written; the kernel's additional random table reads
            # are real traffic but mostly LLC-served (measured, not
            # credited: profiles/r01_q3_kernels_v6 / DESIGN.md §6b).
            "achieved": (24.0 * r["probe_rows"] + 16.0 * r["match_rows"])
                        / (r["probe_ms"] / 1000) / 1e9,
            "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": (24.0 * r["probe_rows"] + 16.0 * r["match_rows"])
                    / (r["probe_ms"] / 1000) / 1e9 / HBM_PEAK_GBPS,
            "traffic": None,
            "kernel": "join probe (count+fill)",
            "kernel_ms": r["probe_ms"],
            "probe_rows": r["probe_rows"], "match_rows": r["match_rows"]},
        "cpu_baseline": None,
    }
    if rank == 0:
        print(json.dumps(out), flush=True)


def run_sweep(args, sess, n_gpus, rank):
    """Implemented-query sweep (BASELINE config 5 shape, the round-1 subset):
    the seven reference-fixture-exact queries back-to-back on one GPU.
    Metric = queries per hour over WALL time (power-run style, including
    per-query input generation); per_query_ms reports each query's own
    pipeline time over HBM-resident inputs (generation excluded, like
    q1/q3's step timing)."""
    from trino_amd import tpch_queries as q
    sf = args.sf_per_gpu

    def run_once(collect):
        for name, fn in (("q1", lambda: _sweep_q1(sess, sf)),
                         ("q2", lambda: q.q2_gpu(sess, sf)),
                         ("q3", lambda: q.q3_gpu(sess, sf)),
                         ("q4", lambda: q.q4_gpu(sess, sf)),
                         ("q5", lambda: q.q5_gpu(sess, sf)),
                         ("q7", lambda: q.q7_gpu(sess, sf)),
                         ("q8", lambda: q.q8_gpu(sess, sf)),
                         ("q6", lambda: q.q6_gpu(sess, sf)),
                         ("q9", lambda: q.q9_gpu(sess, sf)),
                         ("q10", lambda: q.q10_gpu(sess, sf)),
                         ("q11", lambda: q.q11_gpu(sess, sf)),
                         ("q12", lambda: q.q12_gpu(sess, sf)),
                         ("q13", lambda: q.q13_gpu(sess, sf)),
                         ("q14", lambda: q.q14_gpu(sess, sf)),
                         ("q15", lambda: q.q15_gpu(sess, sf)),
                         ("q16", lambda: q.q16_gpu(sess, sf)),
                         ("q17", lambda: q.q17_gpu(sess, sf)),
                         ("q18", lambda: q.q18_gpu(sess, sf)),
                         ("q19", lambda: q.q19_gpu(sess, sf)),
                         ("q20", lambda: q.q20_gpu(sess, sf)),
                         ("q21", lambda: q.q21_gpu(sess, sf)),
                         ("q22", lambda: q.q22_gpu(sess, sf))):
            r = fn()
            collect[name] = collect.get(name, 0.0) + r["elapsed"]

    def _sweep_q1(s, sf):
        import trino_amd
        li = s.tpch_lineitem(sf)
        t0 = time.time()
        s.q1(li)
        el = time.time() - t0
        s.tpch_lineitem_free(li)
        return {"elapsed": el}

    for _ in range(max(args.warmup, 1)):
        run_once({})
    per = {}
    t0 = time.time()
    for _ in range(args.steps):
        run_once(per)
    wall = time.time() - t0
    out = {
        "metric": "tpch_sweep_queries_per_hour",
        "value": 22 * args.steps / wall * 3600, "unit": "queries/h",
        "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": wall * 1000 / args.steps, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": f"TPC-H full 22-query sweep "
                               f"SF{sf:g} on {n_gpus}xMI355X; all reference-"
                               f"fixture-exact at SF1",
                   "per_query_ms": {k: round(v * 1000 / args.steps, 2)
                                    for k, v in per.items()}},
        "roofline": None,
        "cpu_baseline": None,
    }
    if rank == 0:
        print(json.dumps(out), flush=True)





def run_parquet(args, sess, n_gpus, rank):
    """BASELINE config 2 storage wording: scan SF<n> lineitem PARQUET with
    decode + upload + the fused Q1 kernel INSIDE the timed step. Setup
    (untimed) writes the file once via pyarrow (snappy, v1 pages, 4M-row
    row groups — the reference's ParquetWriter defaults); decode is the
    native reader (csrc/parquet.cpp) with columns x row-groups parallelism.
    After the first warmup pass the file sits in the page cache: the step
    measures decode+upload+kernel, not cold disk (stated in config)."""
    import ctypes
    import numpy as np
    import trino_amd
    from trino_amd import _lib, _check, LineitemCols
    from trino_amd import tpch_queries as tq
    from trino_amd.parquet import ParquetFile, read_columns
    sf = args.sf_per_gpu
    path = os.environ.get("TMPDIR", "/tmp") + f"/lineitem_sf{sf:g}.parquet"
    if not os.path.exists(path):
        import pyarrow as pa
        import pyarrow.parquet as pq
        import oracle          # input fabrication only (never in the step)
        t0 = time.time()
        li = oracle.gen_lineitem(sf)
        flags = np.array(["A", "N", "R"])
        stat = np.array(["F", "O"])
        pq.write_table(pa.table({
            "l_shipdate": li["shipdate"], "l_quantity": li["quantity"],
            "l_extendedprice": li["extendedprice"],
            "l_discount": li["discount"], "l_tax": li["tax"],
            "l_returnflag": flags[li["returnflag"]],
            "l_linestatus": stat[li["linestatus"]],
        }), path, compression="snappy", data_page_version="1.0",
            row_group_size=1 << 22)
        log(f"wrote {os.path.getsize(path)/2**20:.0f} MiB parquet in "
            f"{time.time()-t0:.1f}s")
    fsize = os.path.getsize(path)
    names = ("l_shipdate", "l_quantity", "l_extendedprice", "l_discount",
             "l_tax", "l_returnflag", "l_linestatus")

    pf0 = ParquetFile(path, session=sess)
    n = pf0.num_rows
    pf0.close()
    d = {k: tq._device_buffer(sess, n * sz) for k, sz in
         (("shipdate", 4), ("quantity", 8), ("extendedprice", 8),
          ("discount", 8), ("tax", 8), ("returnflag", 1), ("linestatus", 1))}
    _lib.tg_copy_htod.restype = ctypes.c_int
    _lib.tg_copy_htod.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64]

    def step():
        t0 = time.time()
        pf = ParquetFile(path, session=sess)
        out = read_columns(pf, names, session=sess)
        pf.close()
        t_dec = time.time() - t0
        rf_ids, rf_dict = out["l_returnflag"]
        ls_ids, ls_dict = out["l_linestatus"]
        rf_map = np.array([b"ANR".index(x) for x in rf_dict], np.uint8)
        ls_map = np.array([b"FO".index(x) for x in ls_dict], np.uint8)
        rf = rf_map[rf_ids]
        ls = ls_map[ls_ids]
        t1 = time.time()
        host = dict(shipdate=out["l_shipdate"], quantity=out["l_quantity"],
                    extendedprice=out["l_extendedprice"],
                    discount=out["l_discount"], tax=out["l_tax"],
                    returnflag=rf, linestatus=ls)
        for k, a in host.items():
            _check(_lib.tg_copy_htod(sess._h, d[k], a.ctypes.data, a.nbytes))
        t_up = time.time() - t1
        cols = LineitemCols()
        cols.row_count = n
        for k in d:
            setattr(cols, k, d[k])
        r = sess.q1(cols)
        return time.time() - t0, t_dec, t_up, r

    for _ in range(max(args.warmup, 1)):
        step()
    t_start = time.time()
    tot_dec = tot_up = tot_k = 0.0
    for _ in range(args.steps):
        el, t_dec, t_up, res = step()
        tot_dec += t_dec
        tot_up += t_up
        tot_k += res.elapsed_ms / 1000.0
    elapsed = time.time() - t_start
    if args.dump_outputs and rank == 0:
        dump_q1_outputs(args.dump_outputs, res)
    ms = elapsed * 1000 / args.steps
    raw = n * 38
    out_rec = {
        "metric": "tpch_q1_parquet_scan_throughput",
        "value": n / (elapsed / args.steps), "unit": "rows/s",
        "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {
            "workload": f"TPC-H Q1 over SF{sf:g} lineitem PARQUET "
                        f"(snappy, v1 pages): native decode + HtoD upload + "
                        f"fused kernel inside the step; file page-cached "
                        f"after warmup (not cold disk)",
            "parquet_bytes": fsize, "rows_total": n,
            "decode_GBps": raw / (tot_dec / args.steps) / 1e9,
            "upload_GBps": raw / (tot_up / args.steps) / 1e9,
            "decode_ms": tot_dec * 1000 / args.steps,
            "upload_ms": tot_up * 1000 / args.steps,
            "parallelism": "dp1"},
        "roofline": {"bound": "hbm",
                     "achieved": raw / (tot_k / args.steps) / 1e9,
                     "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": raw / (tot_k / args.steps) / 1e9 / HBM_PEAK_GBPS,
                     "traffic": None,
                     "kernel": "q1 fused scan/filter/agg (decode+upload are "
                               "host-side, reported in config)",
                     "kernel_ms": tot_k * 1000 / args.steps},
        "cpu_baseline": None,
    }
    for k in d.values():
        tq._device_free(sess, k)
    if rank == 0:
        print(json.dumps(out_rec), flush=True)


if __name__ == "__main__":
    main()
