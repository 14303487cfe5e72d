"""Cost of the lookup join's residual filter step (filter_matches: pair-filter
kernel, scans, placement), measured with the stream timer.

    python tools/measure_join_filter_cost.py [--steps 15] [--warmup 3]
                                             [--unfiltered-only] [--out FILE]

Same build and page as tools/measure_outer_join_cost.py: a 2^20-row unique
build and ONE device-resident 2^22-row probe page whose rows all hit;
tg_timer_start/stop around add_input, a fresh operator per step (closed
afterwards, so the pool serves every step from its cache).

 1. add_input without a filter, join_type 0..3, interleaved step by step:
    the existing path. --unfiltered-only stops here and uses nothing the
    parent commit lacks, so the same file measures the parent's library.
 2. add_input with the filter probe.x < build.y, inner and LEFT, where y is
    set so that about 0 %, 50 % and 100 % of the pairs pass; the unfiltered
    step of the same join type runs interleaved as the base. The base
    gathers every pair, the filtered step only the survivors, so the
    difference is the filter step minus the gathers it saves; the per-kernel
    split of a rocprofv3 --kernel-trace --stats run separates the two.
 3. the same at 50 % against a duplicate-heavy build (500 copies per key,
    2^20 rows) and a probe page of 2^22 / 500 rows: about 2^22 candidate pairs.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import trino_amd  # noqa: E402
from trino_amd import _check, _lib, ops  # noqa: E402
from trino_amd.tpch_queries import _device_buffer, _device_free, _timed  # noqa: E402

NB, M = 1 << 20, 1 << 22
COPIES = 500
_K = np.int64(-7046029254386353131)
JT = {0: "inner", 1: "left", 2: "right", 3: "full"}


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


def build(s, bk, y):
    """build channels [key, y, row]; output key + row as in the outer tool"""
    bridge = ops.JoinBridge(s)
    b = ops.hash_builder(s, bridge, [ops.TG_BIGINT] * 3, [0], [0, 2])
    b.add_input(ops.page_from_numpy([bk, y, np.arange(len(bk), dtype=np.int64)]))
    b.drain()
    b.close()
    return bridge


def probe_step(s, bridge, page, join_type, flt=None):
    kw = {} if flt is None else {"filter": flt}
    op = ops.lookup_join(s, bridge, [ops.TG_BIGINT] * 3, [0], [0, 2],
                         join_type=join_type, **kw)
    ms = _timed(s, lambda: op.add_input(page))
    op.finish()
    op.close()
    return ms


def interleaved(s, a, variants):
    """variants: name -> (bridge, page, join_type, filter); one step of each
    per round, the order rotating"""
    names = list(variants)
    t = {n: [] for n in names}
    for step in range(a.warmup + a.steps):
        k = step % len(names)
        for n in names[k:] + names[:k]:
            ms = probe_step(s, *variants[n])
            if step >= a.warmup:
                t[n].append(ms)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--unfiltered-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = np.random.default_rng(1)
    bk = (r.permutation(NB).astype(np.int64) + 1) * _K
    pk = bk[r.integers(0, NB, M)]
    x = r.integers(0, 1000, M).astype(np.int64)
    s = trino_amd.Session(0)
    lines = [f"{trino_amd.version()}",
             f"command: python tools/measure_join_filter_cost.py --steps {a.steps} "
             f"--warmup {a.warmup}" + (" --unfiltered-only" if a.unfiltered_only else ""),
             f"build {NB} unique BIGINT keys, channels key, y, row; probe page {M} rows, "
             f"device-resident, all hit, channels key, x, row; output key + row of each "
             f"side (4 x BIGINT per output row)"]
    try:
        page, bufs = device_page(s, [pk, x, np.arange(M, dtype=np.int64)])
        # 1. the existing path: one bridge per recording type keeps the
        # measure_outer_join_cost.py steady state (bits set after step one)
        y_half = np.full(NB, 500, np.int64)
        bridges = {jt: build(s, bk, y_half) for jt in JT}
        t = interleaved(s, a, {jt: (bridges[jt], page, jt, None) for jt in JT})
        for jt in JT:
            lines.append(f"add_input join_type {jt} ({JT[jt]:5s}) no filter : {stats(t[jt])}")
        for b in bridges.values():
            b.close()
        if not a.unfiltered_only:
            flt = ops.expr(("col", 1), ("col", 3 + 1), "lt")      # probe.x < build.y
            for pct, yv in ((0, 0), (50, 500), (100, 1000)):
                y = np.full(NB, yv, np.int64)
                br = {k: build(s, bk, y) for k in ("i", "if", "l", "lf")}
                t = interleaved(s, a, {"i": (br["i"], page, 0, None),
                                       "if": (br["if"], page, 0, flt),
                                       "l": (br["l"], page, 1, None),
                                       "lf": (br["lf"], page, 1, flt)})
                for base, f, name in (("i", "if", "inner"), ("l", "lf", "left ")):
                    d = np.median(t[f]) - np.median(t[base])
                    lines.append(f"filter x < y passing ~{pct:3d} %, {name}: {stats(t[f])}")
                    lines.append(f"    unfiltered base                : {stats(t[base])}")
                    lines.append(f"    filtered minus unfiltered add_input (medians): {d:+.3f} ms = "
                                 f"{1e9 * d / M:.1f} ps per candidate pair")
                for b in br.values():
                    b.close()
            # 3. duplicate-heavy build: 500 copies per key
            nkeys = NB // COPIES
            dk = (np.repeat(np.arange(nkeys), COPIES).astype(np.int64) + 1) * _K
            dk = np.concatenate([dk, (np.arange(nkeys * COPIES, NB).astype(np.int64) + 1) * _K])
            dk = dk[r.permutation(NB)]
            md = M // COPIES
            dpk = (r.integers(0, nkeys, md).astype(np.int64) + 1) * _K
            dpage, dbufs = device_page(s, [dpk, r.integers(0, 1000, md).astype(np.int64),
                                           np.arange(md, dtype=np.int64)])
            br = {k: build(s, dk, np.full(NB, 500, np.int64)) for k in ("i", "if", "l", "lf")}
            t = interleaved(s, a, {"i": (br["i"], dpage, 0, None),
                                   "if": (br["if"], dpage, 0, flt),
                                   "l": (br["l"], dpage, 1, None),
                                   "lf": (br["lf"], dpage, 1, flt)})
            lines.append(f"duplicate-heavy build: {nkeys} keys x {COPIES} copies in {NB} rows, "
                         f"probe page {md} rows = {md * COPIES} candidate pairs, ~50 % pass")
            for base, f, name in (("i", "if", "inner"), ("l", "lf", "left ")):
                d = np.median(t[f]) - np.median(t[base])
                lines.append(f"filter x < y passing ~ 50 %, {name}: {stats(t[f])}")
                lines.append(f"    unfiltered base                : {stats(t[base])}")
                lines.append(f"    filtered minus unfiltered add_input (medians): {d:+.3f} ms = "
                             f"{1e9 * d / (md * COPIES):.1f} ps per candidate pair")
            for b in br.values():
                b.close()
            for p in dbufs:
                _device_free(s, p)
        for p in bufs:
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
