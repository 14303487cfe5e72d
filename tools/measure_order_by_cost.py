"""What the OrderBy operator costs: against the Window on fixed-width keys,
and on VARCHAR keys and payloads, with the kernel-time split of the string
image.

    python tools/measure_order_by_cost.py [--steps 15] [--warmup 3]
        [--case all|fixed|a|b|c|d] [--only all|new]
        [--kernel-stats CASE=FILE:RUNS] [--out FILE]

Every page is device-resident. A fresh operator per step; the stream timer
brackets add_input + finish + the get_output that orders and gathers; the
steps of two contenders alternate.

  fixed  2^24 rows, keys (BIGINT, BIGINT), one BIGINT payload, one page:
         ops.order_by against ops.window with the one ROW_NUMBER spec over the
         same keys as sort keys. Requirement: the OrderBy median is not above
         the Window's median by more than the Window's own run-to-run spread,
         (max - min) / median.
  a      2^22 rows, one VARCHAR key of distinct 10-byte strings that separate
         in their first 8 bytes, a BIGINT payload
  b      2^22 rows, distinct 40-byte strings: a common 32-byte prefix, then 8
         bytes that separate them (five chunk rounds)
  c      2^22 rows, 2^10 distinct 10-byte strings repeated
  d      2^22 rows, a BIGINT key and a VARCHAR payload of 100-byte strings;
         beside it an identity ops.filter_project over the same page, whose
         VARCHAR channel goes through k_gather_var_bytes (run_gather_var)

  sweep  the byte-copy kernels alone: a BIGINT key already in order (so the
         index list is the identity, the same list for both kernels) and a
         VARCHAR payload whose lengths are uniform in [0, 2 x MEAN]
         (--mean 3 | 30 | 100 | 400). order_by runs once per step under
         TG_VAR_COPY_LANES = 1, 2, ..., 64, and the identity filter_project
         runs beside it. Only a profiled run says anything here: its
         kernel stats are read back with --sweep-stats MEAN=FILE (MEANs=FILE
         for a run with --scattered, a shuffled key) and give
         each k_pages_var_copy<LANES> and k_gather_var_bytes in ms and in
         GB/s of bytes moved, with the verdict for the lane count the
         library's table picks.

Kernel times come from a SEPARATE profiled run, one case per run and the new
operator alone (case d: and the identity filter_project), so that the kernel
names do not mix:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o a -- \
        python tools/measure_order_by_cost.py --case a --only new --steps 5 --warmup 0

read back with --kernel-stats a=DIR/.../a_kernel_stats.csv:5 (5 = operator
runs in the profiled process). For case d the two byte-copy kernels are also
printed as GB/s of bytes moved (read + written). Without a GPU the tool
fails; it has no fallback.
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

N_FIXED = 1 << 24
N_VAR = 1 << 22
PAYLOAD_LEN = 100


def summary(ms):
    a = np.sort(np.asarray(ms))
    med = float(np.median(a))
    return med, float(a[0]), float(a[-1])


def stats(ms):
    med, lo, hi = summary(ms)
    return (f"median {med:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   "
            f"spread (max-min)/median {100 * (hi - lo) / med:5.1f} %")


def to_device(s, a, bufs):
    p = _device_buffer(s, max(a.nbytes, 1))
    _check(_lib.tg_copy_htod(s._h, p, a.ctypes.data, a.nbytes))
    bufs.append(p)
    return p.value


def device_page(s, columns, bufs):
    """columns: int64 arrays, or (uint8 byte matrix [n, len]) for a VARCHAR
    channel of equal-length strings"""
    n = len(columns[0])
    blocks = (ops.TgBlock * len(columns))()
    for i, col in enumerate(columns):
        blocks[i].kind = 0
        blocks[i].position_count = n
        blocks[i].on_device = 1
        if isinstance(col, tuple):
            data, offsets = col
            blocks[i].type = ops.TG_VARCHAR
            blocks[i].data = to_device(s, data, bufs)
            blocks[i].offsets = to_device(s, offsets, bufs)
        elif col.dtype == np.uint8:
            offsets = (np.arange(n + 1, dtype=np.int64) * col.shape[1]).astype(np.int32)
            blocks[i].type = ops.TG_VARCHAR
            blocks[i].data = to_device(s, np.ascontiguousarray(col), bufs)
            blocks[i].offsets = to_device(s, offsets, bufs)
        else:
            blocks[i].type = ops.TG_BIGINT
            blocks[i].data = to_device(s, col, bufs)
    p = ops.TgPage()
    p.channel_count = len(columns)
    p.position_count = n
    p.blocks = blocks
    p._keepalive = blocks
    return p


def nibble_strings(values, nibbles, length, prefix=0):
    """[n, length] bytes: `prefix` constant bytes, then the low `nibbles`
    nibbles of each value as letters, most significant first, then padding"""
    out = np.full((len(values), length), ord("."), np.uint8)
    out[:, :prefix] = ord("p")
    for k in range(nibbles):
        out[:, prefix + k] = ord("a") + ((values >> (4 * (nibbles - 1 - k))) & 15)
    return out


def fetch(op):
    out, fin = ops.TgPage(), ctypes.c_int(0)
    _check(_lib.tg_operator_get_output(op._h, ctypes.byref(out), ctypes.byref(fin)))
    return out


def run_op(s, op, page, channels):
    got = {}

    def work():
        op.add_input(page)
        op.finish()
        out = fetch(op)
        got["rows"], got["channels"] = out.position_count, out.channel_count

    ms = _timed(s, work)
    op.close()
    assert got == {"rows": page.position_count, "channels": channels}, got
    return ms


def types_of(page):
    return [page.blocks[i].type for i in range(page.channel_count)]


def run_order_by(s, page, sort):
    op = ops.order_by(s, types_of(page), sort, [0] * len(sort))
    return run_op(s, op, page, page.channel_count)


def run_window(s, page, sort):
    op = ops.window(s, types_of(page), [], sort, [0] * len(sort),
                    [(ops.WIN_ROW_NUMBER, -1, ops.WIN_FRAME_RANGE)])
    return run_op(s, op, page, page.channel_count + 1)


def run_identity_filter_project(s, page):
    ty = types_of(page)
    # an identity projection takes its source's type; the declared one is unused
    declared = [ops.TG_DOUBLE if t == ops.TG_VARCHAR else t for t in ty]
    op = ops.filter_project(s, None, [ops.expr(("col", j)) for j in range(len(ty))], declared)
    return run_op(s, op, page, len(ty))


KERNEL_CLASSES = (("radix sorts (rocPRIM)", r"rocprim::"),
                  ("chunk and length images",
                   r"\bk_var_chunks\b|\bk_var_lens\b|\bk_var_len_image\b|\bk_var_finish\b"),
                  ("flags + scan + scatter",
                   r"\bk_var_flags\b|\bk_var_scatter_ranks\b|\bk_s32_chunk_sums\b|"
                   r"\bk_s32_chunks_serial\b|\bk_s32_offsets\b|\bk_scan_serial\b"),
                  ("new byte copy (k_pages_var_copy)", r"\bk_pages_var_copy<"),
                  ("old byte copy (k_gather_var_bytes)", r"\bk_gather_var_bytes\b"),
                  ("gathers (keys by permutation, payload, lengths)",
                   r"\bk_gather_u64_by_perm\b|\bk_topn_gather<|\bk_pages_var_lens\b|"
                   r"\bk_gather_var_lens\b|\bk_gather<"),
                  ("fixed-width key images, iota",
                   r"\bk_topn_keys\b|\bk_topn_null_keys\b|\bk_iota_i64\b"))


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


def sweep_rows(mean):
    return min(N_VAR, (1 << 29) // mean)


def sweep_page(s, mean, r, bufs, scattered=False):
    n = sweep_rows(mean)
    lens = r.integers(0, 2 * mean + 1, n)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum(lens)
    data = r.integers(ord("a"), ord("z") + 1, int(offsets[n]) + 1, dtype=np.uint8)
    key = r.permutation(n) if scattered else np.arange(n, dtype=np.int64)
    page = device_page(s, [key, (data, offsets)], bufs)
    return page, int(offsets[n])


def table_lanes():
    """the lane table of var_copy_lanes, read from the source"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "trino_amd", "csrc", "sort.hip")).read()
    m = re.search(r"return mean <= (\d+) \? (\d+) : mean <= (\d+) \? (\d+) : "
                  r"mean <= (\d+) \? (\d+) : (\d+);", src)
    v = [int(x) for x in m.groups()]
    return lambda mean: v[1] if mean <= v[0] else v[3] if mean <= v[2] else v[5] if mean <= v[4] else v[6]


def sweep_report(mean, path, moved, label="identity index list"):
    """lines for one --sweep-stats file; moved = bytes read + written per run"""
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            m = re.search(r"\bk_pages_var_copy<(\d+)>", name)
            key = int(m.group(1)) if m else 0 if re.search(r"\bk_gather_var_bytes\b", name) else None
            if key is None:
                continue
            get = lambda *ks: next((float(row[k]) for k in ks if row.get(k)), None)     # noqa: E731
            calls = int(get("Calls") or 1)
            avg = get("AverageNs", "Average(ns)") or get("TotalDurationNs", "TotalDuration(ns)") / calls
            rows.append((key, calls, avg, get("MinNs", "Min(ns)") or avg,
                         get("MaxNs", "Max(ns)") or avg))
    rows.sort()
    out = [f"byte-copy kernels alone, mean length {mean}: {sweep_rows(mean)} rows, {label}, "
           f"{moved / 1e9:.3f} GB read + written per launch (rocprofv3 --kernel-trace --stats)"]
    old = None
    for key, calls, avg, lo, hi in rows:
        label = "k_gather_var_bytes (old)" if key == 0 else f"k_pages_var_copy<{key}>"
        out.append(f"    {label:28s} {calls:3d} launches  mean {avg / 1e6:8.4f} ms  min {lo / 1e6:8.4f}  "
                   f"max {hi / 1e6:8.4f}  {moved / avg:8.1f} GB/s")
        if key == 0:
            old = (avg, lo, hi)
    pick = table_lanes()(mean)
    mine = next((r_ for r_ in rows if r_[0] == pick), None)
    best = min((r_ for r_ in rows if r_[0]), key=lambda r_: r_[2], default=None)
    if old and mine:
        spread = (old[2] - old[1]) / old[0]
        verdict = "met" if mine[2] <= old[0] * (1 + spread) else "NOT met"
        out.append(f"    the table picks {pick} lanes: {mine[2] / old[0]:.3f} of the old kernel's time; requirement "
                   f"(not slower than the old kernel beyond its spread {100 * spread:.1f} %): {verdict}; "
                   f"fastest lane count measured: {best[0]} ({best[2] / 1e6:.4f} ms)")
    return out


def build_case(s, case, r, bufs):
    """(page, sort channels, description)"""
    if case == "fixed":
        cols = [r.integers(0, 1 << 12, N_FIXED), r.integers(0, 1 << 40, N_FIXED),
                r.integers(-(1 << 30), 1 << 30, N_FIXED)]
        return device_page(s, cols, bufs), [0, 1], (
            f"fixed: {N_FIXED} rows, keys (BIGINT, BIGINT), one BIGINT payload, one page")
    n = N_VAR
    rid = np.arange(n, dtype=np.int64)
    if case == "a":
        key = nibble_strings(r.permutation(n), 6, 10)
        what = "a: distinct 10-byte strings that separate in their first 8 bytes"
    elif case == "b":
        key = nibble_strings(r.permutation(n), 6, 40, prefix=32)
        what = "b: distinct 40-byte strings, a common 32-byte prefix then 8 distinct bytes"
    elif case == "c":
        key = nibble_strings(r.integers(0, 1 << 10, n), 3, 10)
        what = "c: 2^10 distinct 10-byte strings repeated"
    else:
        pay = r.integers(ord("a"), ord("z") + 1, (n, PAYLOAD_LEN), dtype=np.uint8)
        return device_page(s, [r.integers(0, 1 << 40, n), pay], bufs), [0], (
            f"d: {n} rows, a BIGINT key and a {PAYLOAD_LEN}-byte VARCHAR payload")
    return device_page(s, [key, rid], bufs), [0], f"{what}; {n} rows, a BIGINT payload"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=("all", "fixed", "a", "b", "c", "d", "sweep", "none"), default="all",
                    help="none: only read --kernel-stats / --sweep-stats files back (no GPU needed)")
    ap.add_argument("--mean", type=int, default=100, help="case sweep: mean payload length")
    ap.add_argument("--scattered", action="store_true",
                    help="case sweep: a shuffled key, so order_by's index list is scattered "
                         "(the identity filter_project beside it keeps its identity list)")
    ap.add_argument("--sweep-stats", action="append", default=[],
                    help="MEAN=FILE, a rocprofv3 kernel stats csv of a profiled run of this script "
                         "with --case sweep --mean MEAN")
    ap.add_argument("--only", choices=("all", "new"), default="all",
                    help="new: without the Window of case fixed (for a profiled run)")
    ap.add_argument("--kernel-stats", action="append", default=[],
                    help="CASE=FILE:RUNS, a rocprofv3 kernel stats csv of a profiled run of "
                         "this script with --case CASE --only new and RUNS operator runs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    cases = ("fixed", "a", "b", "c", "d") if a.case == "all" else (a.case,)
    r = np.random.default_rng(1)
    if a.case == "none":
        cases = ()
    s = trino_amd.Session(0) if a.case != "none" else None      # fails here without a GPU
    lines = [f"{trino_amd.version()}",
             f"command: python tools/measure_order_by_cost.py --steps {a.steps} "
             f"--warmup {a.warmup} --case {a.case} --only {a.only}"]
    try:
        if a.case == "sweep":
            cases = ()
            bufs = []
            page, total = sweep_page(s, a.mean, r, bufs, a.scattered)
            for step in range(a.warmup + a.steps):
                for lanes in (1, 2, 4, 8, 16, 32, 64):
                    os.environ["TG_VAR_COPY_LANES"] = str(lanes)
                    run_order_by(s, page, [0])
                del os.environ["TG_VAR_COPY_LANES"]
                run_identity_filter_project(s, page)
            lines.append(f"sweep: mean {a.mean}, {page.position_count} rows, {total} payload bytes; "
                         f"read the profiled run's kernel stats with --sweep-stats")
            for p in bufs:
                _device_free(s, p)
        for case in cases:
            bufs = []
            page, sort, what = build_case(s, case, r, bufs)
            new, other = [], []
            for step in range(a.warmup + a.steps):
                ms = run_order_by(s, page, sort)
                if step >= a.warmup:
                    new.append(ms)
                if case == "fixed" and a.only == "all":
                    ms = run_window(s, page, sort)
                elif case == "d":
                    ms = run_identity_filter_project(s, page)
                else:
                    continue
                if step >= a.warmup:
                    other.append(ms)
            lines.append(what)
            lines.append(f"  order_by                      : {stats(new)}")
            if case == "fixed" and other:
                lines.append(f"  window (ROW_NUMBER, same keys) : {stats(other)}")
                nm, wm = summary(new)[0], summary(other)
                spread = (wm[2] - wm[1]) / wm[0]
                verdict = "met" if nm <= wm[0] * (1 + spread) else "NOT met"
                lines.append(f"  order_by / window = {nm / wm[0]:.3f}; requirement (order_by median <= window "
                             f"median x (1 + its spread {100 * spread:.1f} %)): {verdict}")
            if case == "d":
                lines.append(f"  identity filter_project       : {stats(other)}")
            for p in bufs:
                _device_free(s, p)
    finally:
        if s is not None:
            s.close()
    for item in a.kernel_stats:
        case, rest = item.split("=", 1)
        path, runs = rest.rsplit(":", 1)
        runs = int(runs)
        per = read_kernel_stats(path)
        total = sum(per.values())
        lines.append(f"kernel time per run, case {case} (rocprofv3 --kernel-trace --stats, separate "
                     f"run, {runs} operator runs): all kernels {total / runs / 1e6:.3f} ms")
        for name, ns in per.items():
            if ns:
                lines.append(f"    {name:48s} {ns / runs / 1e6:8.3f} ms  {100 * ns / max(total, 1):5.1f} %")
        if case == "d":
            moved = 2.0 * N_VAR * PAYLOAD_LEN
            for name in ("new byte copy (k_pages_var_copy)", "old byte copy (k_gather_var_bytes)"):
                if per[name]:
                    lines.append(f"    {name}: {moved / 1e9:.3f} GB read + written per run, "
                                 f"{moved / (per[name] / runs):.1f} GB/s")
    for item in a.sweep_stats:
        mean, path = item.split("=", 1)
        label = "identity index list"
        if mean.endswith("s"):
            mean, label = mean[:-1], "order_by through a scattered index list, the old kernel through the identity"
        mean = int(mean)
        r2 = np.random.default_rng(1)           # the page of the profiled run: same seed, same draw
        total = int(r2.integers(0, 2 * mean + 1, sweep_rows(mean)).sum())
        lines += sweep_report(mean, path, 2.0 * total, label)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
