"""What the Window operator's frame layer costs: bounded ROWS frames and the
value functions through tg_window_create_ex, and whether the first entry
point still costs what it did.

    python tools/measure_window_frames_cost.py [--steps 15] [--warmup 3] [--out FILE]
        [--old-path PARENT.txt:CHANGE.txt ...]

The page of tools/measure_window_cost.py: 2^24 device-resident rows, three
BIGINT channels (partition key, sort key, value), once with about 2^20
partitions and once with a single partition. Three spec lists:

    narrow   SUM_I64 + MIN_I64 over ROWS BETWEEN 6 PRECEDING AND CURRENT ROW
    wide     the same over ROWS BETWEEN 1000 PRECEDING AND 1000 FOLLOWING
    values   LAG(x, 1) + FIRST_VALUE(x) under FRAME_RANGE

A fresh operator per step; the stream timer brackets add_input + finish + the
get_output that sorts, scans and gathers (end-to-end ms per run). The level
count is the number of k_win_level launches the MIN makes,
floor(log2(min(frame width, rows))) + 1. No threshold is set on these: they
are the first measured cost of the frame layer.

--old-path takes pairs of files written by `tools/measure_window_cost.py
--config both --out FILE`, the first from a checkout of the parent commit and
the second from this tree, both taken in the same GPU session (alternate them
when there are several pairs). For each pair and partition shape the change's
median may exceed the parent's by no more than the parent run's own spread
(max - min) / median. Without a GPU the tool fails; it has no fallback.
"""
import argparse
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
RB = ops.WIN_FRAME_ROWS_BETWEEN
CONFIGS = (
    ("narrow", "SUM_I64 + MIN_I64, ROWS BETWEEN 6 PRECEDING AND CURRENT ROW",
     [(ops.WIN_SUM_I64, 2, RB, -6, 0, 0), (ops.WIN_MIN_I64, 2, RB, -6, 0, 0)]),
    ("wide", "SUM_I64 + MIN_I64, ROWS BETWEEN 1000 PRECEDING AND 1000 FOLLOWING",
     [(ops.WIN_SUM_I64, 2, RB, -1000, 1000, 0), (ops.WIN_MIN_I64, 2, RB, -1000, 1000, 0)]),
    ("values", "LAG(x, 1) + FIRST_VALUE(x), FRAME_RANGE",
     [(ops.WIN_LAG, 2, ops.WIN_FRAME_RANGE, 0, 0, 1),
      (ops.WIN_FIRST_VALUE, 2, ops.WIN_FRAME_RANGE, 0, 0, 0)]),
)


def level_count(specs, n):
    """k_win_level launches of the specs' MIN / MAX over a frame bounded at
    both ends (0: none of them slides)"""
    out = 0
    for fn, _, frame, start, end, _ in specs:
        if fn not in (ops.WIN_MIN_I64, ops.WIN_MAX_I64) or frame != RB:
            continue
        if start <= -(n - 1) or end >= n - 1:
            continue                      # open at one end: a scan, no levels
        out = max(out, 1 if end < start else min(end - start + 1, n).bit_length())
    return out


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


def one_run(s, page, specs):
    op = ops.window_ex(s, [ops.TG_BIGINT] * 3, [0], [1], [0], specs)
    out, fin = ops.TgPage(), ctypes.c_int(0)

    def work():
        op.add_input(page)
        op.finish()
        _check(_lib.tg_operator_get_output(op._h, ctypes.byref(out), ctypes.byref(fin)))

    ms = _timed(s, work)
    rows, channels = out.position_count, out.channel_count
    op.close()
    assert rows == N and channels == 3 + len(specs), (rows, channels)
    return ms


END_TO_END = re.compile(r"end to end, (.*?)\s*: median\s+([\d.]+) ms\s+min\s+([\d.]+)\s+max\s+([\d.]+)")


def read_old_path(path):
    """{partition shape: (median, min, max)} from a measure_window_cost.py record"""
    got = {}
    for line in open(path):
        m = END_TO_END.search(line)
        if m:
            got[m.group(1)] = tuple(float(v) for v in m.groups()[1:])
    assert got, f"{path}: no 'end to end' line"
    return got


def old_path_lines(pairs):
    lines = ["first entry point (tools/measure_window_cost.py --config both: ROW_NUMBER + SUM_I64 "
             "FRAME_RANGE through tg_window_create), parent commit against this change, same session;",
             "bar: change median <= parent median * (1 + parent spread), spread = (max - min) / median "
             "of the parent run"]
    for r, pair in enumerate(pairs):
        parent_path, change_path = pair.split(":", 1)
        parent, change = read_old_path(parent_path), read_old_path(change_path)
        for shape in parent:
            pm, plo, phi = parent[shape]
            cm, clo, chi = change[shape]
            spread = (phi - plo) / pm
            verdict = "inside" if cm <= pm * (1 + spread) else "OUTSIDE"
            lines.append(f"    pair {r + 1}, {shape:26s}: parent median {pm:7.3f} ms (min {plo:7.3f} "
                         f"max {phi:7.3f}, spread {100 * spread:4.1f} %)   change median {cm:7.3f} ms "
                         f"(min {clo:7.3f} max {chi:7.3f})   change/parent {cm / pm:6.4f}   "
                         f"{verdict} the parent's spread")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--old-path", action="append", default=[],
                    help="PARENT.txt:CHANGE.txt, two measure_window_cost.py records of one session")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    r = np.random.default_rng(1)
    sort_key = r.integers(0, 1 << 40, N)
    value = r.integers(-(1 << 30), 1 << 30, N)
    keys = {"many": r.integers(0, PARTITIONS, N), "single": np.zeros(N, np.int64)}
    label = {"many": f"about {PARTITIONS} partitions", "single": "a single partition"}
    s = trino_amd.Session(0)       # fails here without a GPU
    lines = [f"{trino_amd.version()}",
             f"command: python tools/measure_window_frames_cost.py --steps {a.steps} "
             f"--warmup {a.warmup}",
             f"page: {N} rows, 3 BIGINT channels (partition key, sort key, value), "
             f"device-resident; two specs through tg_window_create_ex; output 5 BIGINT channels"]
    try:
        for shape in ("many", "single"):
            page, bufs = device_page(s, [keys[shape], sort_key, value])
            for name, text, specs in CONFIGS:
                t = []
                for step in range(a.warmup + a.steps):
                    ms = one_run(s, page, specs)
                    if step >= a.warmup:
                        t.append(ms)
                lines.append(f"end to end, {name:6s} ({text}; k_win_level launches "
                             f"{level_count(specs, N)}), {label[shape]:26s}: {stats(t)}")
            for p in bufs:
                _device_free(s, p)
    finally:
        s.close()
    if a.old_path:
        lines += old_path_lines(a.old_path)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
