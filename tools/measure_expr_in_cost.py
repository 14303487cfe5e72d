"""Cost of the IN-list opcode against the OR chain it replaces, and of the
grown interpreter and term kernel on programs that use only the old opcodes,
measured with the stream timer.

    python tools/measure_expr_in_cost.py [--steps 15] [--warmup 3]
                                         [--parent-capable] [--out FILE]

Device-resident pages of 2^24 rows; tg_timer_start/stop around add_input of a
fresh FilterProject operator per step (closed afterwards, so the pool serves
every step from its cache); the variants of one group run interleaved, the
order rotating step by step.

 1. `x IN (8 sizes) AND y <> c` over INTEGER x (sizes 1..50) and y, written as
    the 31-instruction OR chain (interpreter, k_filter_flags) and as IN_LIST
    (k_filter_terms, one-word mask); then IN alone at k = 64 over a span of
    4000 (bitmap form) and k = 4096 sparse (search form), and the k = 8 list
    under NOT, which takes the interpreter's search.
 2. --parent-capable stops before 1 and times only what the parent commit
    can run, so the same file measures the parent's library:
    a Q6-shaped three-term conjunction (k_filter_terms), an interpreter filter
    (k_filter_flags), a five-instruction projection that is not the mulsub
    special case (k_project), and the join filter step at 50 % (the inner case
    of tools/measure_join_filter_cost.py).
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

N = 1 << 24
NB, M = 1 << 20, 1 << 22
_K = np.int64(-7046029254386353131)
SIZES = [49, 14, 23, 45, 19, 3, 36, 9]
_TG = {np.dtype(np.int64): ops.TG_BIGINT, np.dtype(np.int32): ops.TG_INTEGER,
       np.dtype(np.float64): ops.TG_DOUBLE}


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
    page = ops.page_from_device(s, ([(p.value, _TG[a.dtype]) for p, a in zip(bufs, arrays)],
                                    len(arrays[0])))
    return page, bufs


def fp_step(s, page, flt, projs, out_types):
    """add_input of a fresh FilterProject operator; returns (ms, output rows)"""
    op = ops.filter_project(s, None if flt is None else ops.expr(*flt),
                            [ops.expr(*p) for p in projs], out_types)
    ms = _timed(s, lambda: op.add_input(page))
    op.finish()
    out = ops.TgPage()
    fin = ctypes.c_int(0)
    _check(_lib.tg_operator_get_output(op._h, ctypes.byref(out), ctypes.byref(fin)))
    rows = out.position_count
    op.close()
    return ms, rows


def join_step(s, bridge, page, flt):
    op = ops.lookup_join(s, bridge, [ops.TG_BIGINT] * 3, [0], [0, 2], join_type=0,
                         filter=ops.expr(*flt))
    ms = _timed(s, lambda: op.add_input(page))
    op.finish()
    op.close()
    return ms, -1


def interleaved(a, variants):
    """variants: name -> callable returning (ms, rows); one step of each per
    round, the order rotating"""
    names = list(variants)
    t = {n: [] for n in names}
    rows = {}
    for step in range(a.warmup + a.steps):
        k = step % len(names)
        for n in names[k:] + names[:k]:
            ms, rows[n] = variants[n]()
            if step >= a.warmup:
                t[n].append(ms)
    return t, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-capable", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = np.random.default_rng(1)
    x = r.integers(1, 51, N).astype(np.int32)
    y = r.integers(0, 25, N).astype(np.int32)
    s = trino_amd.Session(0)
    lines = [f"{trino_amd.version()}",
             f"command: python tools/measure_expr_in_cost.py --steps {a.steps} "
             f"--warmup {a.warmup}" + (" --parent-capable" if a.parent_capable else ""),
             f"pages of {N} rows, device-resident; add_input of a FilterProject operator with "
             f"one identity projection unless stated"]
    ident, ident_t = [(("col", 0),)], [ops.TG_INTEGER]
    try:
        if a.parent_capable:
            d = r.integers(8000, 10600, N).astype(np.int32)          # shipdate-like
            disc = np.round(r.integers(0, 11, N) * 0.01, 2)
            qty = r.integers(1, 51, N).astype(np.float64)
            page, bufs = device_page(s, [d, disc, qty, x])
            q6 = (("col", 0), ("i64", 8766), ("i64", 9130), "between",
                  ("col", 1), ("f64", 0.05), ("f64", 0.07), "between", "and",
                  ("col", 2), ("f64", 24.0), "lt", "and")
            interp = (("col", 0), ("col", 3), "add", ("i64", 2), "mul", ("i64", 18500), "gt")
            proj5 = (("col", 1), ("col", 2), "add", ("f64", 0.5), "mul")
            bk = (r.permutation(NB).astype(np.int64) + 1) * _K
            jp, jbufs = device_page(s, [bk[r.integers(0, NB, M)],
                                        r.integers(0, 1000, M).astype(np.int64),
                                        np.arange(M, dtype=np.int64)])
            bridge = ops.JoinBridge(s)
            b = ops.hash_builder(s, bridge, [ops.TG_BIGINT] * 3, [0], [0, 2])
            b.add_input(ops.page_from_numpy([bk, np.full(NB, 500, np.int64),
                                             np.arange(NB, dtype=np.int64)]))
            b.drain()
            b.close()
            jf = (("col", 1), ("col", 3 + 1), "lt")
            t, rows = interleaved(a, {
                "terms": lambda: fp_step(s, page, q6, ident, ident_t),
                "flags": lambda: fp_step(s, page, interp, ident, ident_t),
                "project": lambda: fp_step(s, page, None, [proj5], [ops.TG_DOUBLE]),
                "join": lambda: join_step(s, bridge, jp, jf)})
            lines.append(f"k_filter_terms  Q6-shaped 3 terms, keeps {rows['terms']:9d} : {stats(t['terms'])}")
            lines.append(f"k_filter_flags  7-inst program,   keeps {rows['flags']:9d} : {stats(t['flags'])}")
            lines.append(f"k_project       5-inst projection, all {rows['project']:9d} : {stats(t['project'])}")
            lines.append(f"join filter x < y ~50 %, inner, {M} candidate pairs  : {stats(t['join'])}")
            bridge.close()
            for p in bufs + jbufs:
                _device_free(s, p)
        else:
            page, bufs = device_page(s, [x, y])
            chain = []
            for i, v in enumerate(SIZES):
                chain += [("col", 0), ("i64", v), "eq"] + (["or"] if i else [])
            tail = [("col", 1), ("i64", 7), "ne", "and"]
            k64 = [int(v) for v in r.choice(4000, 64, replace=False) - 1000]
            k4096 = [int(v) for v in r.choice(1 << 30, 4096, replace=False) - (1 << 29)]
            k4096[:8] = SIZES           # so that rows pass
            t, rows = interleaved(a, {
                "or": lambda: fp_step(s, page, chain + tail, ident, ident_t),
                "in8": lambda: fp_step(s, page, [("col", 0), ("in", SIZES)] + tail, ident, ident_t),
                "in8_alone": lambda: fp_step(s, page, [("col", 0), ("in", SIZES)], ident, ident_t),
                "in64": lambda: fp_step(s, page, [("col", 0), ("in", k64)], ident, ident_t),
                "in4096": lambda: fp_step(s, page, [("col", 0), ("in", k4096)], ident, ident_t),
                "in8_interp": lambda: fp_step(s, page, [("col", 0), ("in", SIZES), "not", "not"] + tail,
                                              ident, ident_t)})
            assert rows["or"] == rows["in8"] == rows["in8_interp"], rows
            lines.append(f"x IN (8) AND y <> c as OR chain, 35 insts (k_filter_flags), keeps {rows['or']} : {stats(t['or'])}")
            lines.append(f"x IN (8) AND y <> c as IN_LIST (k_filter_terms, mask form)          : {stats(t['in8'])}")
            lines.append(f"    IN_LIST / OR chain (medians): {np.median(t['in8']) / np.median(t['or']):.3f}")
            lines.append(f"x IN (8) alone (mask form), keeps {rows['in8_alone']:9d}                      : {stats(t['in8_alone'])}")
            lines.append(f"x IN (64 over a span of 4000) (bitmap form), keeps {rows['in64']:9d}     : {stats(t['in64'])}")
            lines.append(f"x IN (4096 sparse) (search form), keeps {rows['in4096']:9d}                : {stats(t['in4096'])}")
            lines.append(f"NOT NOT x IN (8) AND y <> c (interpreter's search, k_filter_flags)  : {stats(t['in8_interp'])}")
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
