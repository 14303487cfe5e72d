"""Cost of recording matched build rows (lookup join join_type 2 against 0)
and of the lookup-outer emission, measured with the stream timer.

    python tools/measure_outer_join_cost.py [--steps 15] [--warmup 3] [--out FILE]

Probe: a 2^20-row unique build and ONE device-resident 2^22-row probe page
whose rows all hit; tg_timer_start/stop around add_input, a fresh operator
per step (closed afterwards, so the pool serves every step from its cache),
join_type 0 and 2 alternating step by step on two bridges over the same
build (steady state: the bits are set after the first step), then the same
with a fresh bridge per step (every bit still clear). Emission: the same build with every other row matched, a fresh
lookup-outer operator per step, the timer around its first get_output.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import trino_amd  # noqa: E402
from trino_amd import _check, _lib, ops  # noqa: E402
from trino_amd.tpch_queries import _device_buffer, _device_free, _timed  # noqa: E402

NB, M = 1 << 20, 1 << 22
_K = np.int64(-7046029254386353131)


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


def build(s, bk):
    bridge = ops.JoinBridge(s)
    b = ops.hash_builder(s, bridge, [ops.TG_BIGINT] * 2, [0], [0, 1])
    b.add_input(ops.page_from_numpy([bk, np.arange(len(bk), dtype=np.int64)]))
    b.drain()
    b.close()
    return bridge


def probe_step(s, bridge, page, join_type):
    op = ops.lookup_join(s, bridge, [ops.TG_BIGINT] * 2, [0], [0, 1], join_type=join_type)
    ms = _timed(s, lambda: op.add_input(page))
    op.finish()
    op.close()
    return ms


def emission_step(s, bridge):
    op = ops.lookup_outer(s, bridge, [ops.TG_BIGINT] * 2)
    out, fin = ops.TgPage(), ctypes.c_int(0)
    ms = _timed(s, lambda: _check(_lib.tg_operator_get_output(
        op._h, ctypes.byref(out), ctypes.byref(fin))))
    rows = out.position_count
    op.close()
    return ms, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = np.random.default_rng(1)
    bk = (r.permutation(NB).astype(np.int64) + 1) * _K
    pk = bk[r.integers(0, NB, M)]
    s = trino_amd.Session(0)
    lines = [f"{trino_amd.version()}",
             f"command: python tools/measure_outer_join_cost.py --steps {a.steps} "
             f"--warmup {a.warmup}",
             f"build {NB} unique BIGINT keys; probe page {M} rows, device-resident, all hit; "
             f"probe and build output: key + row (4 x BIGINT per output row)"]
    try:
        page, bufs = device_page(s, [pk, np.arange(M, dtype=np.int64)])
        bridges = {0: build(s, bk), 2: build(s, bk)}
        t = {0: [], 2: []}
        for step in range(a.warmup + a.steps):
            for jt in ((0, 2) if step % 2 == 0 else (2, 0)):
                ms = probe_step(s, bridges[jt], page, jt)
                if step >= a.warmup:
                    t[jt].append(ms)
        lines.append(f"add_input join_type 0 (inner)      : {stats(t[0])}")
        lines.append(f"add_input join_type 2 (recording)  : {stats(t[2])}")
        d = np.median(t[2]) - np.median(t[0])
        lines.append(f"recording cost (difference of medians): {d:.3f} ms = "
                     f"{100 * d / np.median(t[0]):.1f} % of the inner add_input, "
                     f"{1e9 * d / M:.1f} ps per match; bits already set after the "
                     f"first step, so the plain load skips the atomics "
                     f"(k_mark_visited: wave-combined, skip-if-set variant; the "
                     f"per-match atomic variant was not built)")
        for b in bridges.values():
            b.close()
        # the bridges above keep their bitmap: after the first step every bit
        # is set and the plain load skips all atomics. A fresh bridge per step
        # (built outside the timer) makes every step set all 2^20 bits anew.
        # join_type 0 gets a fresh bridge too, so both see the same cold table.
        cold = {0: [], 2: []}
        for step in range(a.warmup + a.steps):
            for jt in ((0, 2) if step % 2 == 0 else (2, 0)):
                fresh = build(s, bk)
                ms = probe_step(s, fresh, page, jt)
                fresh.close()
                if step >= a.warmup:
                    cold[jt].append(ms)
        lines.append(f"fresh bridge per step, join_type 0 : {stats(cold[0])}")
        lines.append(f"fresh bridge per step, join_type 2 : {stats(cold[2])}")
        dc = np.median(cold[2]) - np.median(cold[0])
        lines.append(f"recording cost with every bit still clear: {dc:.3f} ms = "
                     f"{100 * dc / np.median(cold[0]):.1f} % of the inner add_input "
                     f"(includes allocating and zeroing the {NB // 8} byte bitmap)")
        # emission: every other build row matched
        half = build(s, bk)
        hp, hbufs = device_page(s, [bk[0::2].copy(), np.arange(NB // 2, dtype=np.int64)])
        probe_step(s, half, hp, 2)
        e = []
        for step in range(a.warmup + a.steps):
            ms, rows = emission_step(s, half)
            assert rows == NB // 2, rows
            if step >= a.warmup:
                e.append(ms)
        lines.append(f"lookup-outer get_output, {NB // 2} of {NB} rows unmatched "
                     f"(2 NULL + 2 gathered BIGINT columns): {stats(e)}")
        half.close()
        for p in bufs + hbufs:
            _device_free(s, p)
    finally:
        s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
