"""What the TopNRanking operator costs against the composition it replaces,
how its kernel time splits, and which compaction threshold is fastest.

    python tools/measure_topn_ranking_cost.py [--steps 15] [--warmup 3] [--config both]
        [--only all|new] [--kernel-stats many=FILE:RUNS] [--kernel-stats single=FILE:RUNS]
        [--out FILE]

The page of tools/measure_window_cost.py: 2^24 device-resident rows, three
BIGINT channels (partition key, sort key, value), once with about 2^20
partitions and once with a single partition. Three measurements per
configuration, all in this process and under one protocol (a fresh operator
per step, the stream timer around add_input + finish + get_output, the steps
of the two contenders alternating):

  new          ops.topn_ranking, ROW_NUMBER, N = 10, emit_ranking, one page
  composition  ops.window with the one ROW_NUMBER spec, then
               ops.filter_project with rn <= 10 over the Window's device page
  threshold    the new operator fed the same rows as 16 pages of 2^20 rows
               under TG_TOPNR_COMPACT_ROWS = 2^20, 2^22 and 2^24

The requirement printed at the end of each configuration: the new operator's
median is not above the composition's median by more than the composition's
own run-to-run spread, (max - min) / median.

Kernel times come from a SEPARATE profiled run, one configuration per run and
the new operator alone, so that the kernel names do not mix:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o many -- \
        python tools/measure_topn_ranking_cost.py --config many --only new --steps 5 --warmup 0

read back with --kernel-stats many=DIR/.../many_kernel_stats.csv:5 (5 =
operator runs in the profiled process). Without a GPU the tool fails; it has
no fallback.
"""
import argparse
import csv
import ctypes
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import trino_amd  # noqa: E402
from trino_amd import _check, _lib, ops  # noqa: E402
from trino_amd.tpch_queries import _device_buffer, _device_free, _timed  # noqa: E402

N = 1 << 24
PARTITIONS = 1 << 20
LIMIT = 10
SPLIT_PAGES = 16
THRESHOLDS = (1 << 20, 1 << 22, 1 << 24)
ENV = "TG_TOPNR_COMPACT_ROWS"
B3 = [ops.TG_BIGINT] * 3


def summary(ms):
    a = np.sort(np.asarray(ms))
    med = float(np.median(a))
    return med, float(a[0]), float(a[-1])


def stats(ms):
    med, lo, hi = summary(ms)
    return (f"median {med:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   "
            f"spread (max-min)/median {100 * (hi - lo) / med:5.1f} %")


def device_pages(s, arrays, pieces):
    """the arrays on the device, as one page and as `pieces` equal pages"""
    bufs = []
    for a in arrays:
        p = _device_buffer(s, a.nbytes)
        _check(_lib.tg_copy_htod(s._h, p, a.ctypes.data, a.nbytes))
        bufs.append(p)
    n = len(arrays[0])
    whole = ops.page_from_device(s, ([(p.value, ops.TG_BIGINT) for p in bufs], n))
    per = n // pieces
    split = [ops.page_from_device(s, ([(p.value + 8 * k * per, ops.TG_BIGINT) for p in bufs], per))
             for k in range(pieces)]
    return whole, split, bufs


def fetch(op):
    out, fin = ops.TgPage(), ctypes.c_int(0)
    _check(_lib.tg_operator_get_output(op._h, ctypes.byref(out), ctypes.byref(fin)))
    return out


def run_new(s, pages, threshold=None):
    """(ms, rows kept) of one fresh TopNRanking operator over `pages`"""
    old = os.environ.get(ENV)
    if threshold is not None:
        os.environ[ENV] = str(threshold)
    try:
        op = ops.topn_ranking(s, B3, [0], [1], [0], ops.RANKING_ROW_NUMBER, LIMIT, True)
    finally:
        if threshold is not None:
            if old is None:
                del os.environ[ENV]
            else:
                os.environ[ENV] = old
    got = {}

    def work():
        for page in pages:
            op.add_input(page)
        op.finish()
        out = fetch(op)
        got["rows"], got["channels"] = out.position_count, out.channel_count

    ms = _timed(s, work)
    op.close()
    assert got["channels"] == 4, got
    return ms, got["rows"]


def run_composition(s, page):
    """(ms, rows kept) of Window(ROW_NUMBER) then FilterProject(rn <= LIMIT)"""
    win = ops.window(s, B3, [0], [1], [0], [(ops.WIN_ROW_NUMBER, -1, ops.WIN_FRAME_RANGE)])
    fp = ops.filter_project(s, ops.expr(("col", 3), ("i64", LIMIT), "le"),
                            [ops.expr(("col", j)) for j in range(4)], [ops.TG_BIGINT] * 4)
    got = {}

    def work():
        win.add_input(page)
        win.finish()
        mid = fetch(win)
        fp.add_input(mid)
        fp.finish()
        out = fetch(fp)
        got["rows"], got["channels"] = out.position_count, out.channel_count

    ms = _timed(s, work)
    fp.close()
    win.close()
    assert got["channels"] == 4, got
    return ms, got["rows"]


KERNEL_CLASSES = (("radix sort (rocPRIM)", r"rocprim|radix|onesweep|sort"),
                  ("key images and boundary flags",
                   r"k_topn_keys|k_topn_null_keys|k_iota|k_win_boundaries"),
                  ("segmented scans (k_wscan_*)", r"k_wscan_"),
                  ("rank cut (k_rcut_*)", r"k_rcut_"),
                  ("gathers (keys by permutation, kept payload)",
                   r"k_gather_u64_by_perm|k_topn_gather"))


def read_kernel_stats(path):
    """{class: total ns} from a rocprofv3 *_kernel_stats.csv"""
    out = {name: 0.0 for name, _ in KERNEL_CLASSES}
    out["other kernels"] = 0.0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            kname = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            for name, pat in KERNEL_CLASSES:
                if re.search(pat, kname):
                    out[name] += ns
                    break
            else:
                out["other kernels"] += ns
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=("many", "single", "both"), default="both")
    ap.add_argument("--only", choices=("all", "new"), default="all",
                    help="new: the new operator's one-page runs alone (for a profiled run)")
    ap.add_argument("--kernel-stats", action="append", default=[],
                    help="CONFIG=FILE:RUNS, a rocprofv3 kernel stats csv of a profiled run of "
                         "this script with --config CONFIG --only new and RUNS operator runs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    r = np.random.default_rng(1)
    sort_key = r.integers(0, 1 << 40, N)
    value = r.integers(-(1 << 30), 1 << 30, N)
    keys = {"many": r.integers(0, PARTITIONS, N), "single": np.zeros(N, np.int64)}
    label = {"many": f"about {PARTITIONS} partitions", "single": "a single partition"}
    configs = ("many", "single") if a.config == "both" else (a.config,)
    s = trino_amd.Session(0)       # fails here without a GPU
    lines = [f"{trino_amd.version()}",
             f"command: python tools/measure_topn_ranking_cost.py --steps {a.steps} "
             f"--warmup {a.warmup} --config {a.config} --only {a.only}",
             f"page: {N} rows, 3 BIGINT channels (partition key, sort key, value), "
             f"device-resident; ROW_NUMBER, N = {LIMIT}; output 4 BIGINT channels"]
    try:
        for cfg in configs:
            whole, split, bufs = device_pages(s, [keys[cfg], sort_key, value], SPLIT_PAGES)
            new, comp = [], []
            by_threshold = {t: [] for t in THRESHOLDS}
            rows = {}
            for step in range(a.warmup + a.steps):
                ms, rows["new"] = run_new(s, [whole])
                if step >= a.warmup:
                    new.append(ms)
                if a.only == "new":
                    continue
                ms, rows["composition"] = run_composition(s, whole)
                if step >= a.warmup:
                    comp.append(ms)
                for t in THRESHOLDS:
                    ms, rows[t] = run_new(s, split, t)
                    if step >= a.warmup:
                        by_threshold[t].append(ms)
            assert len(set(rows.values())) == 1, rows       # everyone keeps the same rows
            lines.append(f"{label[cfg]}: {rows['new']} rows kept")
            lines.append(f"  new operator, one page        : {stats(new)}")
            if a.only == "new":
                for p in bufs:
                    _device_free(s, p)
                continue
            lines.append(f"  composition (window + filter) : {stats(comp)}")
            nm, cm = summary(new)[0], summary(comp)
            spread = (cm[2] - cm[1]) / cm[0]
            verdict = "met" if nm <= cm[0] * (1 + spread) else "NOT met"
            lines.append(f"  new / composition = {nm / cm[0]:.3f}; requirement (new median <= composition "
                         f"median x (1 + its spread {100 * spread:.1f} %)): {verdict}")
            for t in THRESHOLDS:
                lines.append(f"  new operator, {SPLIT_PAGES} pages, {ENV}={t:9d}: "
                             f"{stats(by_threshold[t])}")
            for p in bufs:
                _device_free(s, p)
    finally:
        s.close()
    for item in a.kernel_stats:
        cfg, rest = item.split("=", 1)
        path, runs = rest.rsplit(":", 1)
        runs = int(runs)
        per = read_kernel_stats(path)
        total = sum(per.values())
        lines.append(f"kernel time per run of the new operator, {label[cfg]} (rocprofv3 --kernel-trace "
                     f"--stats, separate run, {runs} operator runs): all kernels "
                     f"{total / runs / 1e6:.3f} ms")
        for name, ns in per.items():
            lines.append(f"    {name:48s} {ns / runs / 1e6:8.3f} ms  {100 * ns / max(total, 1):5.1f} %")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
