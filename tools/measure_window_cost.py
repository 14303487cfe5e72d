"""What the Window operator costs, and how the time splits between sort,
segmented scan and gather.

    python tools/measure_window_cost.py [--steps 15] [--warmup 3] [--config both]
        [--kernel-stats many=FILE:RUNS] [--kernel-stats single=FILE:RUNS] [--out FILE]

One device-resident 2^24-row page with three BIGINT channels (partition key,
sort key, value); specs ROW_NUMBER and SUM_I64 under FRAME_RANGE; once with
about 2^20 partitions and once with a single partition. A fresh operator per
step; the stream timer brackets add_input + finish + the get_output that
sorts, scans and gathers (end-to-end ms per run).

Kernel times come from a SEPARATE profiled run of this same script, one
configuration per run so that the kernel names do not mix:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o many -- \
        python tools/measure_window_cost.py --config many --steps 5 --warmup 0

and are read back with --kernel-stats many=DIR/.../many_kernel_stats.csv:5
(5 = operator runs in the profiled process). The k_wscan_* time per run is
set against the scan's algorithmic bytes, computed below from the shapes, as
a share of the HBM peak. Without a GPU the tool fails; it has no fallback.
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
SPECS = [(ops.WIN_ROW_NUMBER, -1, ops.WIN_FRAME_RANGE), (ops.WIN_SUM_I64, 2, ops.WIN_FRAME_RANGE)]
HBM_PEAK_SPEC = 8.0e12        # MI355X_MICROARCH.md: HBM3E peak BW, spec
HBM_PEAK_MEASURED = 6.29e12   # same table: float4 copy


def scan_constants():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "trino_amd", "csrc", "ops_window.hip")).read()
    return (int(re.search(r"#define WSCAN_CHUNK (\d+)", src).group(1)),
            int(re.search(r"#define WSCAN_ONE_WAVE (\d+)", src).group(1)))


def scan_bytes(n, value_bytes, chunk, one_wave):
    """algorithmic bytes of one run_wscan over n rows whose value source
    reads value_bytes per row: every launch reads value + 1 flag byte per
    row, the applying launch also writes 8; the carries (1 + 8 bytes each)
    are written once, scanned by the same rule and read once"""
    if n <= one_wave:
        return n * (value_bytes + 1 + 8)
    nchunks = -(-n // chunk)
    reduce_ = n * (value_bytes + 1) + nchunks * 9
    apply_ = n * (value_bytes + 1 + 8) + nchunks * 8
    return reduce_ + scan_bytes(nchunks, 8, chunk, one_wave) + apply_


def operator_scan_bytes(n):
    """the scans ROW_NUMBER + SUM_I64/RANGE make (ops_window.hip emit_into):
    row_number (constant 1: no value read), the running non-NULL count of the
    input (one i64 array), the NULL-neutralised running sum (value and
    non-NULL arrays) and the reverse index scan of the peer-group ends (no
    value read)"""
    chunk, one_wave = scan_constants()
    return sum(scan_bytes(n, vb, chunk, one_wave) for vb in (0, 8, 16, 0))


def stats(ms):
    a = np.sort(np.asarray(ms))
    return (f"median {np.median(a):8.3f} ms   min {a[0]:8.3f}   max {a[-1]:8.3f}   "
            f"spread (max-min)/median {100 * (a[-1] - a[0]) / np.median(a):5.1f} %")


def device_page(s, arrays):
    bufs = []
    for a in arrays:
        p = _device_buffer(s, a.nbytes)
        _check(_lib.tg_copy_htod(s._h, p, a.ctypes.data, a.nbytes))
        bufs.append(p)
    page = ops.page_from_device(s, ([(p.value, ops.TG_BIGINT) for p in bufs], len(arrays[0])))
    return page, bufs


def one_run(s, page):
    op = ops.window(s, [ops.TG_BIGINT] * 3, [0], [1], [0], SPECS)
    out, fin = ops.TgPage(), ctypes.c_int(0)

    def work():
        op.add_input(page)
        op.finish()
        _check(_lib.tg_operator_get_output(op._h, ctypes.byref(out), ctypes.byref(fin)))

    ms = _timed(s, work)
    rows, channels = out.position_count, out.channel_count
    op.close()
    assert rows == N and channels == 5, (rows, channels)
    return ms


KERNEL_CLASSES = (("segmented scan (k_wscan_*)", r"k_wscan_"),
                  ("radix sort (rocPRIM)", r"rocprim|radix|onesweep|sort"),
                  ("key images and boundary flags", r"k_topn_keys|k_topn_null_keys|k_iota|k_win_boundaries"),
                  ("gathers (keys by permutation, payload, input, frame ends)",
                   r"k_gather_u64_by_perm|k_topn_gather|k_win_gather_input|k_win_emit"))


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
    ap.add_argument("--kernel-stats", action="append", default=[],
                    help="CONFIG=FILE:RUNS, a rocprofv3 kernel stats csv of a profiled run "
                         "of this script with --config CONFIG and RUNS operator runs")
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
    scan_b = operator_scan_bytes(N)
    s = trino_amd.Session(0)       # fails here without a GPU
    lines = [f"{trino_amd.version()}",
             f"command: python tools/measure_window_cost.py --steps {a.steps} "
             f"--warmup {a.warmup} --config {a.config}",
             f"page: {N} rows, 3 BIGINT channels (partition key, sort key, value), "
             f"device-resident; specs ROW_NUMBER + SUM_I64 FRAME_RANGE; output 5 BIGINT channels",
             f"segmented scans per run: 4 (row_number, non-NULL count, sum, peer-group ends); "
             f"algorithmic bytes {scan_b} = {scan_b / N:.1f} B/row"]
    try:
        for cfg in configs:
            page, bufs = device_page(s, [keys[cfg], sort_key, value])
            t = []
            for step in range(a.warmup + a.steps):
                ms = one_run(s, page)
                if step >= a.warmup:
                    t.append(ms)
            lines.append(f"end to end, {label[cfg]:26s}: {stats(t)}")
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
        lines.append(f"kernel time per run, {label[cfg]} (rocprofv3 --kernel-trace --stats, "
                     f"separate run, {runs} operator runs): all kernels {total / runs / 1e6:.3f} ms")
        for name, ns in per.items():
            lines.append(f"    {name:58s} {ns / runs / 1e6:8.3f} ms  {100 * ns / max(total, 1):5.1f} %")
        scan_s = per[KERNEL_CLASSES[0][0]] / runs / 1e9
        if scan_s > 0:
            rate = scan_b / scan_s
            lines.append(f"    segmented scan: {scan_b} B / {scan_s * 1e3:.3f} ms = {rate / 1e12:.3f} TB/s "
                         f"= {100 * rate / HBM_PEAK_SPEC:.1f} % of the 8.0 TB/s HBM peak (spec), "
                         f"{100 * rate / HBM_PEAK_MEASURED:.1f} % of the 6.29 TB/s measured copy rate; "
                         f"the bound is bytes over bandwidth (one integer operation per row)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
