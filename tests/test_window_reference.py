"""References for the Window operator (trino_amd/csrc/ops_window.hip) and
their own checks. No GPU.

ref_window is plain Python: a stable `sorted` over (partition cells under the
ASC rule, then topn_sort_key of the sort cells), then one sequential pass per
partition. ref_window_vec is its numpy twin for the large shapes of
tests/test_gpu_window_matrix.py: np.lexsort on canonicalised keys,
segment-reset cumulative operations and np.maximum.accumulate on segment
starts. The two are asserted equal on seeded random inputs; a dozen
hand-written tables with typed-out outputs pin ref_window independently, and
the pair operator the device scan rests on is checked associative by brute
force. The scan's chunk constants are parsed out of the source and pinned to
what the GPU matrix assumes.
"""
import itertools
import math
import os
import re

import numpy as np
import pytest

(ROW_NUMBER, RANK, DENSE_RANK, COUNT_STAR, COUNT_COL, SUM_I64, MIN_I64, MAX_I64) = range(8)
RANGE, ROWS, PARTITION = range(3)
FN_NAMES = ("row_number", "rank", "dense_rank", "count_star", "count_col", "sum", "min", "max")
FRAME_NAMES = ("range", "rows", "partition")

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "trino_amd", "csrc")


def wrap64(v):
    return ((v + 2 ** 63) % 2 ** 64) - 2 ** 63


def has_validity(fn):
    """SUM / MIN / MAX outputs carry a bitmap, everything else has none"""
    return fn >= SUM_I64


# --------------------------------------------------------------------------
# the plain reference
# --------------------------------------------------------------------------
def ref_window(rows, partition_channels, sort_channels, sort_desc, specs):
    """rows: tuples of cells (None = NULL). Returns (order, columns): the
    output row order as input row indices and, per spec, the output column as
    a list in output order (None = NULL)."""
    from test_gpu_ordering_matrix import canon_key, topn_sort_key

    def pcells(i):
        return tuple(rows[i][c] for c in partition_channels)

    def scells(i):
        return tuple(rows[i][c] for c in sort_channels)

    asc = [0] * len(partition_channels)
    order = sorted(range(len(rows)),
                   key=lambda i: topn_sort_key(pcells(i), asc) + topn_sort_key(scells(i), sort_desc))
    cols = [[] for _ in specs]
    at = 0
    while at < len(order):
        pk = canon_key(pcells(order[at]))
        stop = at
        while stop < len(order) and canon_key(pcells(order[stop])) == pk:
            stop += 1
        part = order[at:stop]
        at = stop
        # peer groups of the partition
        first_peer, last_peer, group_no = [], [], []
        g = 0
        for r, i in enumerate(part):
            if r and canon_key(scells(i)) == canon_key(scells(part[r - 1])):
                first_peer.append(first_peer[-1])
            else:
                first_peer.append(r)
                g += 1
            group_no.append(g)
        last_peer = [0] * len(part)
        for r in range(len(part) - 1, -1, -1):
            same = r + 1 < len(part) and first_peer[r + 1] == first_peer[r]
            last_peer[r] = last_peer[r + 1] if same else r
        for k, (fn, ch, frame) in enumerate(specs):
            if fn == ROW_NUMBER:
                cols[k] += [r + 1 for r in range(len(part))]
                continue
            if fn == RANK:
                cols[k] += [f + 1 for f in first_peer]
                continue
            if fn == DENSE_RANK:
                cols[k] += group_no
                continue
            running, cnt, acc = [], 0, None
            for r, i in enumerate(part):
                v = None if fn == COUNT_STAR else rows[i][ch]
                if fn == COUNT_STAR:
                    running.append(r + 1)
                    continue
                if v is not None:
                    v = int(v)
                    cnt += 1
                    acc = (v if acc is None else wrap64(acc + v) if fn == SUM_I64
                           else min(acc, v) if fn == MIN_I64 else max(acc, v))
                running.append(cnt if fn == COUNT_COL else acc)
            for r in range(len(part)):
                e = r if frame == ROWS else last_peer[r] if frame == RANGE else len(part) - 1
                cols[k].append(running[e])
    return order, cols


# --------------------------------------------------------------------------
# the vectorised twin
# --------------------------------------------------------------------------
def _canon_arrays(col, desc):
    """(null rank, NaN rank, value) arrays that order like topn_sort_key and
    are equal exactly where canon_key is"""
    n = len(col.values)
    null = np.zeros(n, bool) if col.valid is None else ~col.valid
    if col.kind == "f64":
        v = col.values.astype(np.float64)
        nan = np.isnan(v) & ~null
        v = np.where(null | nan, 0.0, v) + 0.0            # -0.0 -> 0.0
        v = -v + 0.0 if desc else v
    else:
        v = col.values.astype(np.int64)
        nan = np.zeros(n, bool)
        v = np.where(null, 0, v)
        v = ~v if desc else v                              # order-reversing, no overflow
        v = np.where(null, 0, v)
    if desc:     # NULL first, then NaN, then values downwards
        return [(~null).astype(np.int8), (~(nan | null)).astype(np.int8), v]
    return [null.astype(np.int8), nan.astype(np.int8), v]


def _seg_cumsum(x, start):
    """inclusive cumulative sum that restarts where the segment starts;
    `start` is each row's segment-start index; wraps like int64"""
    cs = np.cumsum(x.astype(np.uint64))
    return (cs - (cs[start] - x.astype(np.uint64)[start])).view(np.int64)


def _seg_cummax(x, present, seg_id, start):
    """inclusive running max over present cells, restarting per segment.
    Values are replaced by their 1-based rank among all values (0 = absent),
    offset by the segment number, so np.maximum.accumulate never reaches back
    over a segment start"""
    uniq, inv = np.unique(x, return_inverse=True)
    rank = np.where(present, inv.reshape(-1) + 1, 0).astype(np.int64)
    width = len(uniq) + 1
    acc = np.maximum.accumulate(seg_id * width + rank) - seg_id * width
    return uniq[np.maximum(acc, 1) - 1]


def ref_window_vec(cols, partition_channels, sort_channels, sort_desc, specs):
    """cols: Col objects (kind, values, valid). Returns (order, columns) with
    columns as (int64 values, bool valid or None) in output order."""
    n = len(cols[0].values)
    idx = np.arange(n, dtype=np.int64)
    pkeys = [a for c in partition_channels for a in _canon_arrays(cols[c], 0)]
    skeys = [a for c, d in zip(sort_channels, sort_desc) for a in _canon_arrays(cols[c], d)]
    keys = pkeys + skeys
    order = np.lexsort(keys[::-1]) if keys else idx.copy()   # stable, last key primary

    def starts(arrs):
        s = np.zeros(n, bool)
        s[0] = True
        for a in arrs:
            a = a[order]
            s[1:] |= a[1:] != a[:-1]
        return s

    part_start = starts(pkeys)
    peer_start = part_start | starts(skeys)
    pstart = np.maximum.accumulate(np.where(part_start, idx, 0))
    gstart = np.maximum.accumulate(np.where(peer_start, idx, 0))
    seg_id = np.cumsum(part_start) - 1

    def seg_end(start_flags):
        last = np.ones(n, bool)
        last[:-1] = start_flags[1:]
        return np.minimum.accumulate(np.where(last, idx, n)[::-1])[::-1]

    end = {ROWS: idx, RANGE: seg_end(peer_start), PARTITION: seg_end(part_start)}
    row_number = idx - pstart + 1
    out = []
    for fn, ch, frame in specs:
        if fn == ROW_NUMBER:
            out.append((row_number, None))
            continue
        if fn == RANK:
            out.append((gstart - pstart + 1, None))
            continue
        if fn == DENSE_RANK:
            out.append((_seg_cumsum(peer_start.astype(np.int64), pstart), None))
            continue
        e = end[frame]
        if fn == COUNT_STAR:
            out.append((row_number[e], None))
            continue
        src = cols[ch]
        present = (np.ones(n, bool) if src.valid is None else src.valid)[order]
        x = src.values.astype(np.int64)[order]
        count = _seg_cumsum(present.astype(np.int64), pstart)
        if fn == COUNT_COL:
            out.append((count[e], None))
            continue
        if fn == SUM_I64:
            run = _seg_cumsum(np.where(present, x, 0), pstart)
        elif fn == MAX_I64:
            run = _seg_cummax(x, present, seg_id, pstart)
        else:
            run = ~_seg_cummax(~x, present, seg_id, pstart)      # min(x) = ~max(~x)
        valid = count[e] > 0
        out.append((np.where(valid, run[e], 0), valid))
    return order, out


def as_arrays(ref_cols, specs):
    """ref_window's lists as (int64 values, valid or None), NULL cells 0"""
    out = []
    for col, (fn, _, _) in zip(ref_cols, specs):
        vals = np.array([0 if v is None else v for v in col], np.int64)
        if has_validity(fn):
            out.append((vals, np.array([v is not None for v in col], bool)))
        else:
            assert None not in col
            out.append((vals, None))
    return out


ALL_SPECS = ([(ROW_NUMBER, -1, RANGE), (RANK, -1, RANGE), (DENSE_RANK, -1, RANGE)] +
             [(fn, -1 if fn == COUNT_STAR else 2, fr)
              for fn in (COUNT_STAR, COUNT_COL, SUM_I64, MIN_I64, MAX_I64)
              for fr in (RANGE, ROWS, PARTITION)])


def assert_same(got, exp, specs, what):
    """(order, columns) of one reference or of the device against another"""
    assert np.array_equal(np.asarray(got[0]), np.asarray(exp[0])), f"{what}: row order"
    for k, ((gv, gm), (ev, em)) in enumerate(zip(got[1], exp[1])):
        name = f"{what}: spec {k} {FN_NAMES[specs[k][0]]}/{FRAME_NAMES[specs[k][2]]}"
        assert (gm is None) == (em is None), f"{name}: bitmap presence"
        if em is not None:
            bad = np.flatnonzero(gm != em)
            assert len(bad) == 0, f"{name}: validity at output row {bad[0]}"
        ok = np.ones(len(ev), bool) if em is None else em
        bad = np.flatnonzero((np.asarray(gv) != ev) & ok)
        assert len(bad) == 0, (f"{name}: output row {bad[0]} got {gv[bad[0]]} "
                               f"expected {ev[bad[0]]}")


# --------------------------------------------------------------------------
# vec == plain on random inputs
# --------------------------------------------------------------------------
def random_cols(n, seed, pkind, skind):
    """[partition key, sort key, i64 input (30 % NULL), i16 input, row id];
    few distinct key values, NULL / NaN / -0.0 among them"""
    from test_gpu_filter_matrix import Col, _NP
    r = np.random.default_rng(seed)

    def key(kind, distinct):
        if kind == "f64":
            pool = np.array([0.0, -0.0, math.nan, -math.nan, math.inf, -math.inf, 1.5, -2.25,
                             5e-324], np.float64)
        elif kind == "bool":
            pool = np.array([0, 1], np.int8)
        else:
            info = np.iinfo(_NP[kind])
            pool = np.array([info.min, info.max, 0, -1, 1, 7, -7, 100, -100], _NP[kind])
        vals = pool[r.integers(0, min(distinct, len(pool)), n)]
        return Col(kind, vals, r.random(n) >= 0.15)

    x = r.integers(-1000, 1000, n)
    extreme = r.random(n) < 0.05
    x = np.where(extreme, np.where(r.random(n) < 0.5, I64_MIN, I64_MAX), x)
    return [key(pkind, 6), key(skind, 9), Col("i64", x, r.random(n) >= 0.3),
            Col("i16", r.integers(-300, 300, n), r.random(n) >= 0.5),
            Col("i64", np.arange(n))]


@pytest.mark.parametrize("n", [1, 2, 65, 700, 3001])
@pytest.mark.parametrize("pkind,skind,desc", [("i64", "f64", 0), ("f64", "i32", 1),
                                              ("bool", "i8", 1), ("i16", "f64", 1)])
def test_vec_equals_plain(n, pkind, skind, desc):
    from test_gpu_filter_matrix import rows_of
    cols = random_cols(n, 100 + n, pkind, skind)
    rows = rows_of(cols)
    for pch, sch, sd in (([0], [1], [desc]), ([], [1], [desc]), ([0], [], []), ([], [], []),
                         ([0, 1], [1, 3], [1 - desc, desc])):
        specs = ALL_SPECS + [(SUM_I64, 3, RANGE), (MIN_I64, 3, ROWS), (COUNT_COL, 3, PARTITION)]
        order, plain = ref_window(rows, pch, sch, sd, specs)
        vec = ref_window_vec(cols, pch, sch, sd, specs)
        assert_same(vec, (order, as_arrays(plain, specs)), specs, f"{pch}{sch}{sd}")


# --------------------------------------------------------------------------
# hand-written tables
# --------------------------------------------------------------------------
NAN = math.nan
TABLES = {
    # peers: RANGE takes the value at the group's last row, ROWS its own
    "peers_range_vs_rows": dict(
        rows=[(1, 10, 5), (1, 10, 7), (1, 20, 1), (2, 5, 4)], part=[0], sort=[1], desc=[0],
        specs=[(SUM_I64, 2, RANGE), (SUM_I64, 2, ROWS), (ROW_NUMBER, -1, 0), (RANK, -1, 0),
               (DENSE_RANK, -1, 0)],
        order=[0, 1, 2, 3],
        cols=[[12, 12, 13, 4], [5, 12, 13, 4], [1, 2, 3, 1], [1, 1, 3, 1], [1, 1, 2, 1]]),
    # a frame prefix with no non-NULL input: SUM and MIN are NULL, COUNT_COL is 0
    "all_null_prefix": dict(
        rows=[(1, 1, None), (1, 2, None), (1, 3, 4), (1, 4, None)], part=[0], sort=[1], desc=[0],
        specs=[(SUM_I64, 2, ROWS), (COUNT_COL, 2, ROWS), (MIN_I64, 2, ROWS),
               (COUNT_STAR, -1, ROWS), (SUM_I64, 2, PARTITION), (COUNT_COL, 2, PARTITION)],
        order=[0, 1, 2, 3],
        cols=[[None, None, 4, 4], [0, 0, 1, 1], [None, None, 4, 4], [1, 2, 3, 4],
              [4, 4, 4, 4], [1, 1, 1, 1]]),
    # NULL is a partition value and sorts last
    "null_partition_last": dict(
        rows=[(None, 1), (2, 1), (None, 2), (1, 1)], part=[0], sort=[1], desc=[0],
        specs=[(ROW_NUMBER, -1, 0), (COUNT_STAR, -1, PARTITION)],
        order=[3, 1, 0, 2], cols=[[1, 1, 1, 2], [1, 1, 2, 2]]),
    # DESC: NULL first, and the two NULLs are peers
    "desc_null_first": dict(
        rows=[(3,), (None,), (5,), (None,), (3,)], part=[], sort=[0], desc=[1],
        specs=[(RANK, -1, 0), (DENSE_RANK, -1, 0), (ROW_NUMBER, -1, 0)],
        order=[1, 3, 2, 0, 4], cols=[[1, 1, 3, 4, 4], [1, 1, 2, 3, 3], [1, 2, 3, 4, 5]]),
    # no sort channel: the whole partition is one peer group
    "no_sort_channels": dict(
        rows=[(2, 1), (1, 10), (2, 2), (1, 20), (2, 3)], part=[0], sort=[], desc=[],
        specs=[(RANK, -1, 0), (DENSE_RANK, -1, 0), (ROW_NUMBER, -1, 0), (SUM_I64, 1, RANGE),
               (SUM_I64, 1, ROWS)],
        order=[1, 3, 0, 2, 4],
        cols=[[1] * 5, [1] * 5, [1, 2, 1, 2, 3], [30, 30, 6, 6, 6], [10, 30, 1, 3, 6]]),
    # no partition channel: one partition of everything
    "no_partition_channels": dict(
        rows=[(3,), (1,), (2,), (1,)], part=[], sort=[0], desc=[0],
        specs=[(ROW_NUMBER, -1, 0), (RANK, -1, 0), (MAX_I64, 0, ROWS), (MIN_I64, 0, RANGE),
               (COUNT_STAR, -1, RANGE)],
        order=[1, 3, 2, 0],
        cols=[[1, 2, 3, 4], [1, 1, 3, 4], [1, 1, 2, 3], [1, 1, 1, 1], [2, 2, 3, 4]]),
    # neither: input order, one partition, one peer group
    "no_channels_at_all": dict(
        rows=[(4,), (None,), (-2,)], part=[], sort=[], desc=[],
        specs=[(ROW_NUMBER, -1, 0), (RANK, -1, 0), (SUM_I64, 0, ROWS), (SUM_I64, 0, RANGE),
               (MIN_I64, 0, ROWS), (MAX_I64, 0, PARTITION), (COUNT_COL, 0, RANGE)],
        order=[0, 1, 2],
        cols=[[1, 2, 3], [1, 1, 1], [4, 4, 2], [2, 2, 2], [4, 4, -2], [4, 4, 4], [2, 2, 2]]),
    # grouping equality on a DOUBLE partition key: -0.0 is 0.0, the NaNs are one
    # value above every number, NULL after them
    "double_partition_key": dict(
        rows=[(NAN,), (-0.0,), (0.0,), (-NAN,), (None,), (1.5,)], part=[0], sort=[], desc=[],
        specs=[(ROW_NUMBER, -1, 0), (COUNT_STAR, -1, PARTITION)],
        order=[1, 2, 5, 0, 3, 4], cols=[[1, 2, 1, 1, 2, 1], [2, 2, 1, 2, 2, 1]]),
    # whole-key ties keep input order
    "ties_keep_input_order": dict(
        rows=[(7, 0), (7, 1), (7, 2), (7, 3)], part=[], sort=[0], desc=[1],
        specs=[(RANK, -1, 0), (COUNT_STAR, -1, ROWS), (SUM_I64, 1, ROWS), (SUM_I64, 1, RANGE)],
        order=[0, 1, 2, 3], cols=[[1] * 4, [1, 2, 3, 4], [0, 1, 3, 6], [6] * 4]),
    # INT64 extremes: MIN / MAX keep them, SUM wraps
    "int64_extremes": dict(
        rows=[(I64_MAX,), (1,), (I64_MIN,)], part=[], sort=[], desc=[],
        specs=[(SUM_I64, 0, ROWS), (MIN_I64, 0, ROWS), (MAX_I64, 0, ROWS)],
        order=[0, 1, 2],
        cols=[[I64_MAX, I64_MIN, 0], [I64_MAX, 1, I64_MIN], [I64_MAX, I64_MAX, I64_MAX]]),
    # two partition channels, two sort channels in opposite directions
    "two_and_two": dict(
        rows=[(1, 1, 5, 1), (1, 2, 5, 1), (1, 1, 6, 2), (1, 1, 5, 3), (1, 1, 5, 3)],
        part=[0, 1], sort=[2, 3], desc=[1, 0],
        specs=[(ROW_NUMBER, -1, 0), (RANK, -1, 0), (DENSE_RANK, -1, 0)],
        order=[2, 0, 3, 4, 1],
        cols=[[1, 2, 3, 4, 1], [1, 2, 3, 3, 1], [1, 2, 3, 3, 1]]),
    # a partition without any non-NULL input
    "all_null_partition": dict(
        rows=[(1, None), (1, None), (2, 3)], part=[0], sort=[], desc=[],
        specs=[(SUM_I64, 1, PARTITION), (COUNT_COL, 1, PARTITION), (MAX_I64, 1, RANGE)],
        order=[0, 1, 2], cols=[[None, None, 3], [0, 0, 1], [None, None, 3]]),
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_ref_window_by_hand(name):
    t = TABLES[name]
    assert len(t["rows"]) <= 8
    order, cols = ref_window(t["rows"], t["part"], t["sort"], t["desc"], t["specs"])
    assert order == t["order"]
    assert cols == t["cols"]


def table_cols(rows):
    """a hand-written table as Col objects: BIGINT, or DOUBLE where a float
    appears; NULL cells hold 1 (the poison of the filter matrix)"""
    from test_gpu_filter_matrix import Col
    cols = []
    for cells in zip(*rows):
        isf = any(isinstance(v, float) for v in cells)
        vals = np.array([1 if v is None else v for v in cells], np.float64 if isf else np.int64)
        valid = np.array([v is not None for v in cells], bool)
        cols.append(Col("f64" if isf else "i64", vals, None if valid.all() else valid))
    return cols


@pytest.mark.parametrize("name", sorted(TABLES))
def test_ref_window_vec_by_hand(name):
    t = TABLES[name]
    got = ref_window_vec(table_cols(t["rows"]), t["part"], t["sort"], t["desc"], t["specs"])
    assert_same(got, (t["order"], as_arrays(t["cols"], t["specs"])), t["specs"], name)


# --------------------------------------------------------------------------
# the pair operator of the device scan
# --------------------------------------------------------------------------
def pair_op(op, a, b):
    """(f1,v1) (+) (f2,v2) = (f1|f2, f2 ? v2 : op(v1,v2))"""
    return (a[0] | b[0], b[1] if b[0] else op(a[1], b[1]))


OPS = {"add": lambda x, y: wrap64(x + y), "min": min, "max": max}


@pytest.mark.parametrize("name", sorted(OPS))
def test_pair_operator_is_associative(name):
    op = OPS[name]
    pairs = [(f, v) for f in (0, 1) for v in (-3, -1, 0, 2, 5, I64_MIN, I64_MAX)]
    for a, b, c in itertools.product(pairs, repeat=3):
        assert pair_op(op, pair_op(op, a, b), c) == pair_op(op, a, pair_op(op, b, c)), (a, b, c)


@pytest.mark.parametrize("name", sorted(OPS))
def test_chunked_scan_shape_equals_sequential(name):
    """the three-launch shape in miniature (chunk 4, one 'wave' up to 3
    carries, so 13+ rows recurse): chunk reduce, scan of the carries by the
    same operator, chunk pass with the incoming carry == a sequential scan"""
    op = OPS[name]
    ident = {"add": 0, "min": I64_MAX, "max": I64_MIN}[name]

    def sequential(pairs):
        out, run = [], (0, ident)
        for p in pairs:
            run = pair_op(op, run, p)
            out.append(run)
        return out

    def chunked(pairs, chunk=4, one_wave=3):
        if len(pairs) <= one_wave:
            return sequential(pairs)
        chunks = [pairs[i:i + chunk] for i in range(0, len(pairs), chunk)]
        carries = chunked([sequential(c)[-1] for c in chunks])
        out = []
        for c, rows in enumerate(chunks):
            run = carries[c - 1] if c else (0, ident)
            for p in rows:
                run = pair_op(op, run, p)
                out.append(run)
        return out

    r = np.random.default_rng(5)
    for n in (1, 3, 4, 5, 12, 13, 17, 49, 50, 64):
        for share in (0.0, 0.1, 0.5, 1.0):
            pairs = [(1 if i == 0 or r.random() < share else 0, int(r.integers(-9, 9)))
                     for i in range(n)]
            assert [v for _, v in chunked(pairs)] == [v for _, v in sequential(pairs)], (n, share)


@pytest.mark.parametrize("name", sorted(OPS))
def test_wave_scan_with_ballot_heads_equals_sequential(name):
    """wscan_chunk's 64-row group in miniature (8 lanes): the values take the
    log-step shuffles alone; the flag half of the pair is replaced by
    `start`, the lane of the nearest head at or before a lane (from one
    ballot), and a step combines only while `lane - off >= start`"""
    op = OPS[name]
    lanes = 8
    r = np.random.default_rng(6)
    for heads in range(1 << lanes):
        vals = [int(x) for x in r.integers(-9, 9, lanes)]
        carry = int(r.integers(-9, 9))
        start = [max([j for j in range(l + 1) if heads >> j & 1], default=-1)
                 for l in range(lanes)]
        v = list(vals)
        off = 1
        while off < lanes:
            prev = list(v)
            for l in range(lanes):
                if l >= off and l - off >= start[l]:
                    v[l] = op(prev[l - off], v[l])
            off <<= 1
        v = [op(carry, x) if start[l] < 0 else x for l, x in enumerate(v)]
        run, exp = (0, carry), []
        for l in range(lanes):
            run = pair_op(op, run, (heads >> l & 1, vals[l]))
            exp.append(run[1])
        assert v == exp, (bin(heads), vals, carry)


# --------------------------------------------------------------------------
# constants
# --------------------------------------------------------------------------
def source_constants():
    text = open(os.path.join(_CSRC, "ops_window.hip")).read()

    def one(pat):
        m = re.search(pat, text)
        assert m, pat
        return int(m.group(1))

    return dict(WSCAN_CHUNK=one(r"#define WSCAN_CHUNK (\d+)"),
                WSCAN_ONE_WAVE=one(r"#define WSCAN_ONE_WAVE (\d+)"))


def test_scan_constants_match_the_gpu_matrix():
    import test_gpu_window_matrix as m
    k = source_constants()
    assert k["WSCAN_CHUNK"] == m.WSCAN_CHUNK and k["WSCAN_ONE_WAVE"] == m.WSCAN_ONE_WAVE
    assert k["WSCAN_CHUNK"] % 64 == 0
    # more carries than one wave takes: the carry scan itself runs as three launches
    deep = k["WSCAN_CHUNK"] * k["WSCAN_ONE_WAVE"] + 1
    assert m.DEEP_ROWS == deep <= 2 ** 21
    # the level above the recursion fits one wave again
    assert -(-deep // k["WSCAN_CHUNK"]) // k["WSCAN_CHUNK"] + 1 <= k["WSCAN_ONE_WAVE"]
    c = k["WSCAN_CHUNK"]
    assert m.EDGE_SIZES == (1, 2, 63, 64, 65, c - 1, c, c + 1, 2 * c + 1)
    assert m.WAVE_CARRIES_ROWS == 64 * c + 1
    assert m.page_sizes(deep) == (1, 0, deep - 2, 1)
    # the one-wave path and the three-launch path are both among the edge sizes
    assert any(n <= k["WSCAN_ONE_WAVE"] for n in m.EDGE_SIZES)
    assert any(n > k["WSCAN_ONE_WAVE"] for n in m.EDGE_SIZES)


def test_ops_constants_match_the_header():
    """trino_amd.ops WIN_* against include/trino_gpu.h and this file"""
    header = open(os.path.join(_ROOT, "include", "trino_gpu.h")).read()
    from trino_amd import ops
    for name, val in (("ROW_NUMBER", ROW_NUMBER), ("RANK", RANK), ("DENSE_RANK", DENSE_RANK),
                      ("COUNT_STAR", COUNT_STAR), ("COUNT_COL", COUNT_COL),
                      ("SUM_I64", SUM_I64), ("MIN_I64", MIN_I64), ("MAX_I64", MAX_I64),
                      ("FRAME_RANGE", RANGE), ("FRAME_ROWS", ROWS),
                      ("FRAME_PARTITION", PARTITION)):
        m = re.search(rf"TG_WIN_{name} = (\d+)", header)
        assert m and int(m.group(1)) == val == getattr(ops, f"WIN_{name}"), name
    import ctypes
    assert ctypes.sizeof(ops.TgWindowSpec) == 16
