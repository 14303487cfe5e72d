"""References for the Window operator's frame layer (tg_window_create_ex in
trino_amd/csrc/ops_window.hip: bounded ROWS frames, lag / lead / first_value /
last_value / nth_value) and their own checks. No GPU.

ref_window_ex is plain Python written from the contract in
include/trino_gpu.h: the ordering and the partition / peer rules of
ref_window, then per row the frame [lo, hi] and a walk over its cells.
ref_window_ex_vec is its numpy twin for the large shapes of
tests/test_gpu_window_frames_matrix.py: counts and sums are differences of
int64 cumulative sums, min / max over a frame open at one end is a segmented
running max, and min / max over a frame bounded at both ends pads every
partition with identities and takes fixed-width block prefix / suffix maxima
(van Herk / Gil-Werman), which shares nothing with the device's level loop.
The two are asserted equal on seeded random inputs at every frame of FRAMES;
hand-written tables pin ref_window_ex independently; the two identities the
kernels rest on (the wrapping prefix difference and the two-window
sparse-table query) are checked by brute force; a numpy model of the bounds
kernel's saturating arithmetic is set against Python's unbounded integers.

A spec here is (fn, input_channel, frame, frame_start, frame_end, offset).
"""
import math
import os
import re

import numpy as np
import pytest

from test_window_reference import (ALL_SPECS, COUNT_COL, COUNT_STAR, DENSE_RANK, I64_MAX,
                                   I64_MIN, MAX_I64, MIN_I64, PARTITION, RANGE, RANK,
                                   ROW_NUMBER, ROWS, SUM_I64, _canon_arrays, _seg_cummax,
                                   as_arrays, random_cols, ref_window, wrap64)

LAG, LEAD, FIRST_VALUE, LAST_VALUE, NTH_VALUE = range(8, 13)
ROWS_BETWEEN = 3
UNB_P, UNB_F = I64_MIN, I64_MAX
FN_NAMES = ("row_number", "rank", "dense_rank", "count_star", "count_col", "sum", "min", "max",
            "lag", "lead", "first_value", "last_value", "nth_value")
FRAME_NAMES = ("range", "rows", "partition", "rows_between")

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every ROWS BETWEEN frame of the GPU matrix: frame lengths at 2^k - 1, 2^k and
# 2^k + 1 around the wave (64) and the scan chunk (1024), frames open at one
# end and at both, always-empty frames, offsets that only saturation survives
FRAMES = ((0, 0), (-1, 0), (0, 1), (-1, 1), (-6, 0), (-3, -1), (2, 5), (3, 1),
          (-63, 0), (-64, 0), (-32, 32), (-1023, 0), (-1024, 0), (-700, 700),
          (UNB_P, 0), (UNB_P, 3), (UNB_P, -2), (-3, UNB_F), (2, UNB_F), (UNB_P, UNB_F),
          (-2 ** 62, 2 ** 62), (I64_MIN + 1, I64_MAX - 1))


def ex(fn, ch=-1, frame=RANGE, start=0, end=0, offset=0):
    return (fn, ch, frame, start, end, offset)


def widen(specs):
    """(fn, ch, frame) specs of the first entry point as specs of the second"""
    return [ex(fn, ch, fr) for fn, ch, fr in specs]


def is_value_fn(fn):
    return fn >= LAG


def has_validity_ex(fn):
    """SUM / MIN / MAX and every value function carry a bitmap"""
    return fn >= SUM_I64


def spec_name(sp):
    fn, ch, frame, start, end, offset = sp
    return f"{FN_NAMES[fn]}({ch},{offset})/{FRAME_NAMES[frame]}[{start},{end}]"


# --------------------------------------------------------------------------
# the plain reference
# --------------------------------------------------------------------------
def frame_of(r, m, last_peer, frame, start, end):
    """[lo, hi] of the row at position r of a partition of m rows, in
    partition-local positions (ps = 0, pe = m - 1). Python integers do not
    wrap, which is what 'the sum saturates' asks for."""
    if frame == RANGE:
        return 0, last_peer[r]
    if frame == ROWS:
        return 0, r
    if frame == PARTITION:
        return 0, m - 1
    return max(0, r + start), min(m - 1, r + end)


def ref_window_ex(rows, partition_channels, sort_channels, sort_desc, specs):
    """rows: tuples of cells (None = NULL). Returns (order, columns) like
    ref_window; a value function's column holds the copied cells."""
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
        m = len(part)
        first_peer, group_no = [], []
        g = 0
        for r, i in enumerate(part):
            if r and canon_key(scells(i)) == canon_key(scells(part[r - 1])):
                first_peer.append(first_peer[-1])
            else:
                first_peer.append(r)
                g += 1
            group_no.append(g)
        last_peer = [0] * m
        for r in range(m - 1, -1, -1):
            same = r + 1 < m and first_peer[r + 1] == first_peer[r]
            last_peer[r] = last_peer[r + 1] if same else r
        for k, (fn, ch, frame, start, end, offset) in enumerate(specs):
            if fn == ROW_NUMBER:
                cols[k] += [r + 1 for r in range(m)]
                continue
            if fn == RANK:
                cols[k] += [f + 1 for f in first_peer]
                continue
            if fn == DENSE_RANK:
                cols[k] += group_no
                continue
            cells = None if fn == COUNT_STAR else [rows[i][ch] for i in part]
            for r in range(m):
                if fn == LAG:
                    cols[k].append(cells[r - offset] if r - offset >= 0 else None)
                    continue
                if fn == LEAD:
                    cols[k].append(cells[r + offset] if r + offset <= m - 1 else None)
                    continue
                lo, hi = frame_of(r, m, last_peer, frame, start, end)
                if fn == COUNT_STAR:
                    cols[k].append(max(0, hi - lo + 1))
                elif lo > hi:                       # the empty frame
                    cols[k].append(0 if fn == COUNT_COL else None)
                elif fn == FIRST_VALUE:
                    cols[k].append(cells[lo])
                elif fn == LAST_VALUE:
                    cols[k].append(cells[hi])
                elif fn == NTH_VALUE:
                    cols[k].append(cells[lo + offset - 1] if lo + offset - 1 <= hi else None)
                else:
                    seen = [int(v) for v in cells[lo:hi + 1] if v is not None]
                    if fn == COUNT_COL:
                        cols[k].append(len(seen))
                    elif not seen:
                        cols[k].append(None)
                    elif fn == SUM_I64:
                        acc = 0
                        for v in seen:
                            acc = wrap64(acc + v)
                        cols[k].append(acc)
                    else:
                        cols[k].append(min(seen) if fn == MIN_I64 else max(seen))
    return order, cols


def cells_as_bits(cells, kind):
    """a value column as int64: DOUBLE cells by their bits, NULL cells 0"""
    from test_gpu_filter_matrix import _NP
    filled = [0 if v is None else v for v in cells]
    if kind == "f64":
        return np.array(filled, np.float64).view(np.int64)
    return np.array(filled, _NP[kind]).astype(np.int64)


def as_arrays_ex(ref_cols, specs, kinds):
    """ref_window_ex's lists as (int64 values, valid or None), NULL cells 0;
    kinds: the kind of every input channel"""
    out = []
    for col, sp in zip(ref_cols, specs):
        if is_value_fn(sp[0]):
            out.append((cells_as_bits(col, kinds[sp[1]]), np.array([v is not None for v in col], bool)))
        else:
            out += as_arrays([col], [sp[:3]])
    return out


def assert_same_ex(got, exp, specs, what):
    """(order, columns) against (order, columns): order, bitmap presence,
    validity and every valid value"""
    assert np.array_equal(np.asarray(got[0]), np.asarray(exp[0])), f"{what}: row order"
    assert len(got[1]) == len(exp[1]) == len(specs)
    for sp, (gv, gm), (ev, em) in zip(specs, got[1], exp[1]):
        name = f"{what}: {spec_name(sp)}"
        assert (gm is None) == (em is None) == (not has_validity_ex(sp[0])), f"{name}: bitmap presence"
        if em is not None:
            bad = np.flatnonzero(gm != em)
            assert len(bad) == 0, f"{name}: validity at output row {bad[0]}, expected {em[bad[0]]}"
        ok = np.ones(len(ev), bool) if em is None else em
        bad = np.flatnonzero((np.asarray(gv) != ev) & ok)
        assert len(bad) == 0, (f"{name}: output row {bad[0]} got {np.asarray(gv)[bad[0]]} "
                               f"expected {ev[bad[0]]}")


# --------------------------------------------------------------------------
# the vectorised twin
# --------------------------------------------------------------------------
def _running_max(x, present, seg_id, reverse):
    """max of the present cells from the partition start up to each row
    (reverse: from each row to the partition end)"""
    if not reverse:
        return _seg_cummax(x, present, seg_id, None)
    rid = (seg_id[-1] - seg_id)[::-1]
    return _seg_cummax(x[::-1], present[::-1], rid, None)[::-1]


def _block_max(x, present, seg_id, a, b):
    """max of the present cells of [i + a, i + b] cut to the row's partition,
    a <= b: every partition is laid out with max(|a|, |b|) identity cells on
    either side, so each frame is an uncut window of exactly w = b - a + 1
    cells, the maximum of a block-suffix and a block-prefix maximum over
    blocks of w cells"""
    n = len(x)
    pad = max(abs(a), abs(b))
    w = b - a + 1
    q = np.arange(n, dtype=np.int64) + pad * (2 * seg_id + 1)
    total = n + 2 * pad * (int(seg_id[-1]) + 1)
    y = np.full(-(-total // w) * w, I64_MIN, np.int64)
    y[q] = np.where(present, x, I64_MIN)
    blocks = y.reshape(-1, w)
    prefix = np.maximum.accumulate(blocks, axis=1).ravel()
    suffix = np.maximum.accumulate(blocks[:, ::-1], axis=1)[:, ::-1].ravel()
    return np.maximum(suffix[q + a], prefix[q + b])


def ref_window_ex_vec(cols, partition_channels, sort_channels, sort_desc, specs):
    """cols: Col objects. Returns (order, columns), every column as (int64
    values, bool valid or None) in output order, value columns as bits."""
    n = len(cols[0].values)
    idx = np.arange(n, dtype=np.int64)
    pkeys = [a for c in partition_channels for a in _canon_arrays(cols[c], 0)]
    skeys = [a for c, d in zip(sort_channels, sort_desc) for a in _canon_arrays(cols[c], d)]
    keys = pkeys + skeys
    order = np.lexsort(keys[::-1]) if keys else idx.copy()

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

    pend, gend = seg_end(part_start), seg_end(peer_start)
    clip = lambda v: max(-n - 1, min(n + 1, v))          # noqa: E731  (same frames, no overflow)

    def bounds(frame, start, end):
        if frame == RANGE:
            return pstart, gend
        if frame == ROWS:
            return pstart, idx
        if frame == PARTITION:
            return pstart, pend
        return np.maximum(pstart, idx + clip(start)), np.minimum(pend, idx + clip(end))

    def sorted_input(ch):
        src = cols[ch]
        present = (np.ones(n, bool) if src.valid is None else src.valid)[order]
        raw = src.values.view(np.int64) if src.kind == "f64" else src.values.astype(np.int64)
        return raw[order], present

    out = []
    for fn, ch, frame, start, end, offset in specs:
        if fn == ROW_NUMBER:
            out.append((idx - pstart + 1, None))
            continue
        if fn == RANK:
            out.append((gstart - pstart + 1, None))
            continue
        if fn == DENSE_RANK:
            cs = np.cumsum(peer_start.astype(np.int64))
            out.append((cs - cs[pstart] + 1, None))
            continue
        lo, hi = bounds(frame, start, end)
        some = lo <= hi
        if fn == COUNT_STAR:
            out.append((np.where(some, hi - lo + 1, 0), None))
            continue
        x, present = sorted_input(ch)
        if is_value_fn(fn):
            k = clip(offset)
            if fn == LAG:
                at, ok = idx - k, idx - k >= pstart
            elif fn == LEAD:
                at, ok = idx + k, idx + k <= pend
            elif fn == FIRST_VALUE:
                at, ok = lo, some
            elif fn == LAST_VALUE:
                at, ok = hi, some
            else:
                at, ok = lo + k - 1, some & (lo + k - 1 <= hi)
            at = np.where(ok, at, 0)
            ok = ok & present[at]
            out.append((np.where(ok, x[at], 0), ok))
            continue
        # prefix sums with a leading 0: sum over [lo, hi] = P[hi + 1] - P[lo]
        l, h = np.where(some, lo, 0), np.where(some, hi + 1, 0)
        pc = np.concatenate([[0], np.cumsum(present.astype(np.int64))])
        count = pc[h] - pc[l]
        if fn == COUNT_COL:
            out.append((count, None))
            continue
        valid = count > 0
        if fn == SUM_I64:
            ps = np.concatenate([np.zeros(1, np.uint64),
                                 np.cumsum(np.where(present, x, 0).astype(np.uint64))])
            res = (ps[h] - ps[l]).view(np.int64)
        else:
            y = x if fn == MAX_I64 else ~x                    # min(x) = ~max(~x)
            if not some.any():
                res = np.zeros(n, np.int64)
            elif np.array_equal(lo[some], pstart[some]):
                res = _running_max(y, present, seg_id, False)[np.where(some, hi, 0)]
            elif np.array_equal(hi[some], pend[some]):
                res = _running_max(y, present, seg_id, True)[np.where(some, lo, 0)]
            else:
                res = _block_max(y, present, seg_id, clip(start), clip(end))
            res = res if fn == MAX_I64 else ~res
        out.append((np.where(valid, res, 0), valid))
    return order, out


# --------------------------------------------------------------------------
# old specs: ref_window_ex == ref_window
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 65, 700])
@pytest.mark.parametrize("pkind,skind,desc", [("i64", "f64", 0), ("bool", "i8", 1)])
def test_old_specs_equal_ref_window(n, pkind, skind, desc):
    from test_gpu_filter_matrix import rows_of
    cols = random_cols(n, 300 + n, pkind, skind)
    rows = rows_of(cols)
    kinds = [c.kind for c in cols]
    for pch, sch, sd in (([0], [1], [desc]), ([], [1], [desc]), ([0], [], []), ([], [], [])):
        order, old = ref_window(rows, pch, sch, sd, ALL_SPECS)
        order_ex, new = ref_window_ex(rows, pch, sch, sd, widen(ALL_SPECS))
        assert order == order_ex and old == new
        vec = ref_window_ex_vec(cols, pch, sch, sd, widen(ALL_SPECS))
        assert_same_ex(vec, (order, as_arrays_ex(old, widen(ALL_SPECS), kinds)),
                       widen(ALL_SPECS), "old specs")


# --------------------------------------------------------------------------
# vec == plain on random inputs, at every frame
# --------------------------------------------------------------------------
def frame_specs(start, end, x=2, v=1):
    """every aggregate and first / last / nth_value under one frame"""
    return ([ex(fn, -1 if fn == COUNT_STAR else x, ROWS_BETWEEN, start, end)
             for fn in (COUNT_STAR, COUNT_COL, SUM_I64, MIN_I64, MAX_I64)] +
            [ex(FIRST_VALUE, v, ROWS_BETWEEN, start, end), ex(LAST_VALUE, v, ROWS_BETWEEN, start, end),
             ex(NTH_VALUE, v, ROWS_BETWEEN, start, end, 2)])


def value_specs(ch, n):
    ks = (0, 1, 2, 63, 64, 65, 1024, 1025, n - 1, n, 2 ** 62)
    return ([ex(LAG, ch, RANGE, offset=k) for k in ks] + [ex(LEAD, ch, RANGE, offset=k) for k in ks] +
            [ex(fn, ch, fr, offset=o) for fr in (RANGE, ROWS, PARTITION)
             for fn, o in ((FIRST_VALUE, 0), (LAST_VALUE, 0), (NTH_VALUE, 1), (NTH_VALUE, 2),
                           (NTH_VALUE, 65), (NTH_VALUE, 2 ** 62))])


@pytest.mark.parametrize("n", [1, 2, 65, 700, 3000])
@pytest.mark.parametrize("pkind,skind,desc", [("i64", "f64", 0), ("i16", "i32", 1)])
def test_vec_equals_plain_at_every_frame(n, pkind, skind, desc):
    from test_gpu_filter_matrix import rows_of
    cols = random_cols(n, 500 + n, pkind, skind)
    rows = rows_of(cols)
    kinds = [c.kind for c in cols]
    # partitioned everywhere; one partition of everything where the plain walk stays cheap
    shapes = [([0], [1], [desc])] + ([([], [1], [desc])] if n <= 700 else [])
    for pch, sch, sd in shapes:
        specs = [sp for start, end in FRAMES for sp in frame_specs(start, end)] + value_specs(1, n)
        order, plain = ref_window_ex(rows, pch, sch, sd, specs)
        vec = ref_window_ex_vec(cols, pch, sch, sd, specs)
        assert_same_ex(vec, (order, as_arrays_ex(plain, specs, kinds)), specs, f"{pch}{sch}")


def test_block_max_path_is_reached():
    """the bounded frames of the comparison above do take the block prefix /
    suffix form, and a frame cut at both partition edges inside one block is
    among them"""
    r = np.random.default_rng(9)
    n = 300
    x = r.integers(-50, 50, n)
    present = r.random(n) >= 0.3
    seg_id = np.sort(r.integers(0, 40, n))
    seg_id = np.cumsum(np.concatenate([[0], seg_id[1:] != seg_id[:-1]]))
    for a, b in ((-1, 1), (-6, 0), (2, 5), (-32, 32), (-64, 0), (-300, 300)):
        got = _block_max(x, present, seg_id, a, b)
        for i in range(n):
            cells = [int(x[j]) for j in range(max(0, i + a), min(n - 1, i + b) + 1)
                     if seg_id[j] == seg_id[i] and present[j]]
            assert got[i] == (max(cells) if cells else I64_MIN), (a, b, i)


# --------------------------------------------------------------------------
# hand-written tables
# --------------------------------------------------------------------------
RB = ROWS_BETWEEN
NAN = math.nan
FRAME_TABLES = {
    # lag / lead stop at the partition's edges, and k = 0 is the row itself
    "lag_lead_at_partition_edges": dict(
        rows=[(1, 10), (1, 20), (1, None), (2, 40), (2, 50)], part=[0], sort=[], desc=[],
        specs=[ex(LAG, 1, offset=1), ex(LEAD, 1, offset=1), ex(LAG, 1, offset=2),
               ex(LEAD, 1, offset=0), ex(LEAD, 1, offset=2 ** 62)],
        order=[0, 1, 2, 3, 4],
        cols=[[None, 10, 20, None, 40], [20, None, None, 50, None], [None, None, 10, None, None],
              [10, 20, None, 40, 50], [None] * 5]),
    # nth_value past the frame's end is NULL although the partition goes on
    "nth_value_past_the_frame_end": dict(
        rows=[(5,), (6,), (7,), (8,)], part=[], sort=[0], desc=[0],
        specs=[ex(NTH_VALUE, 0, RB, -1, 0, 2), ex(NTH_VALUE, 0, RB, -1, 0, 3),
               ex(NTH_VALUE, 0, ROWS, offset=3), ex(NTH_VALUE, 0, PARTITION, offset=4),
               ex(NTH_VALUE, 0, RB, 0, 1, 1)],
        order=[0, 1, 2, 3],
        cols=[[None, 6, 7, 8], [None] * 4, [None, None, 7, 7], [8] * 4, [5, 6, 7, 8]]),
    # frame_start > frame_end: every frame is empty
    "all_empty_frame": dict(
        rows=[(1,), (2,), (3,)], part=[], sort=[0], desc=[0],
        specs=[ex(COUNT_STAR, -1, RB, 3, 1), ex(COUNT_COL, 0, RB, 3, 1), ex(SUM_I64, 0, RB, 3, 1),
               ex(MIN_I64, 0, RB, 3, 1), ex(FIRST_VALUE, 0, RB, 3, 1), ex(LAST_VALUE, 0, RB, 3, 1),
               ex(NTH_VALUE, 0, RB, 3, 1, 1)],
        order=[0, 1, 2],
        cols=[[0] * 3, [0] * 3, [None] * 3, [None] * 3, [None] * 3, [None] * 3, [None] * 3]),
    # offsets past the partition's edge: empty on some rows only
    "frame_past_the_partition_edge": dict(
        rows=[(1, 1), (1, 2), (1, 3), (2, 9)], part=[0], sort=[1], desc=[0],
        specs=[ex(SUM_I64, 1, RB, 1, 2), ex(COUNT_STAR, -1, RB, 1, 2), ex(MAX_I64, 1, RB, -2, -1),
               ex(LAST_VALUE, 1, RB, 1, 2)],
        order=[0, 1, 2, 3],
        cols=[[5, 3, None, None], [2, 1, 0, 0], [None, 1, 2, None], [3, 3, None, None]]),
    # a frame wider than its partition is the partition
    "frame_wider_than_partition": dict(
        rows=[(1, 4), (1, None), (1, -2), (2, 7)], part=[0], sort=[], desc=[],
        specs=[ex(SUM_I64, 1, RB, -100, 100), ex(MIN_I64, 1, RB, -2 ** 62, 2 ** 62),
               ex(COUNT_COL, 1, RB, I64_MIN + 1, I64_MAX - 1), ex(COUNT_STAR, -1, RB, UNB_P, UNB_F),
               ex(FIRST_VALUE, 1, RB, -100, 100), ex(LAST_VALUE, 1, RB, -100, 100)],
        order=[0, 1, 2, 3],
        cols=[[2, 2, 2, 7], [-2, -2, -2, 7], [2, 2, 2, 1], [3, 3, 3, 1], [4, 4, 4, 7],
              [-2, -2, -2, 7]]),
    # a moving window: NULLs are skipped by the aggregates, kept by first / last
    "moving_window_with_nulls": dict(
        rows=[(3,), (None,), (None,), (1,), (5,)], part=[], sort=[], desc=[],
        specs=[ex(SUM_I64, 0, RB, -1, 0), ex(MIN_I64, 0, RB, -1, 1), ex(MAX_I64, 0, RB, -1, 0),
               ex(COUNT_COL, 0, RB, -1, 1), ex(FIRST_VALUE, 0, RB, -1, 0), ex(LAST_VALUE, 0, RB, 0, 1)],
        order=[0, 1, 2, 3, 4],
        cols=[[3, 3, None, 1, 6], [3, 3, 1, 1, 1], [3, 3, None, 1, 5], [1, 1, 1, 2, 2],
              [3, 3, None, None, 1], [None, None, 1, 5, 5]]),
    # the identity of min / max is a legal value: INT64_MAX next to NULLs
    "identity_is_a_value": dict(
        rows=[(None,), (I64_MAX,), (None,), (I64_MIN,)], part=[], sort=[], desc=[],
        specs=[ex(MIN_I64, 0, RB, 0, 0), ex(MAX_I64, 0, RB, 0, 0), ex(MIN_I64, 0, RB, -1, 0),
               ex(MAX_I64, 0, RB, -1, 1), ex(SUM_I64, 0, RB, -2, 0)],
        order=[0, 1, 2, 3],
        cols=[[None, I64_MAX, None, I64_MIN], [None, I64_MAX, None, I64_MIN],
              [None, I64_MAX, I64_MAX, I64_MIN], [I64_MAX, I64_MAX, I64_MAX, I64_MIN],
              [None, I64_MAX, I64_MAX, -1]]),
    # first / last over the peers frame, DOUBLE cells copied as they are
    "double_cells_and_peers": dict(
        rows=[(1, -0.0), (1, NAN), (2, None), (2, 2.5)], part=[], sort=[0], desc=[0],
        specs=[ex(FIRST_VALUE, 1, RANGE), ex(LAST_VALUE, 1, RANGE), ex(LAST_VALUE, 1, ROWS),
               ex(LAG, 1, offset=1)],
        order=[0, 1, 2, 3],
        cols=[[-0.0] * 4, [NAN, NAN, 2.5, 2.5], [-0.0, NAN, None, 2.5], [None, -0.0, NAN, None]]),
}


def _same_cell(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).view(np.int64) == np.float64(b).view(np.int64)
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("name", sorted(FRAME_TABLES))
def test_ref_window_ex_by_hand(name):
    t = FRAME_TABLES[name]
    order, cols = ref_window_ex(t["rows"], t["part"], t["sort"], t["desc"], t["specs"])
    assert order == t["order"]
    for got, exp, sp in zip(cols, t["cols"], t["specs"]):
        assert len(got) == len(exp) and all(_same_cell(g, e) for g, e in zip(got, exp)), \
            (spec_name(sp), got, exp)


@pytest.mark.parametrize("name", sorted(FRAME_TABLES))
def test_ref_window_ex_vec_by_hand(name):
    from test_window_reference import table_cols
    t = FRAME_TABLES[name]
    cols = table_cols(t["rows"])
    got = ref_window_ex_vec(cols, t["part"], t["sort"], t["desc"], t["specs"])
    exp = as_arrays_ex(t["cols"], t["specs"], [c.kind for c in cols])
    assert_same_ex(got, (t["order"], exp), t["specs"], name)


# --------------------------------------------------------------------------
# the identities the kernels rest on
# --------------------------------------------------------------------------
def random_partition(r, m, nulls):
    vals = [int(v) for v in r.integers(-1000, 1000, m)]
    for j in range(m):
        if r.random() < 0.1:
            vals[j] = I64_MIN if r.random() < 0.5 else I64_MAX
    present = [not nulls or r.random() >= 0.4 for _ in range(m)]
    return vals, present


@pytest.mark.parametrize("nulls", [False, True], ids=["no_nulls", "nulls"])
def test_prefix_difference_is_the_wrapped_frame_sum(nulls):
    """S[hi] - (lo > ps ? S[lo - 1] : 0) in wrapping arithmetic, S the inclusive
    scan that restarts at the partition start, equals the wrapped sequential
    sum of the frame's non-NULL cells; the same difference on the non-NULL
    count is the frame's count"""
    r = np.random.default_rng(21)
    for m in (1, 2, 7, 40):
        vals, present = random_partition(r, m, nulls)
        S, C, acc, cnt = [], [], 0, 0
        for v, p in zip(vals, present):
            acc = wrap64(acc + (v if p else 0))
            cnt += 1 if p else 0
            S.append(acc)
            C.append(cnt)
        for lo in range(m):
            for hi in range(lo, m):
                seq = 0
                for j in range(lo, hi + 1):
                    if present[j]:
                        seq = wrap64(seq + vals[j])
                assert wrap64(S[hi] - (S[lo - 1] if lo > 0 else 0)) == seq, (m, lo, hi)
                assert C[hi] - (C[lo - 1] if lo > 0 else 0) == sum(present[lo:hi + 1])


@pytest.mark.parametrize("nulls", [False, True], ids=["no_nulls", "nulls"])
@pytest.mark.parametrize("name", ["min", "max"])
def test_two_window_query_is_the_frame_min_max(name, nulls):
    """T_0 = cells with NULLs as the identity, T_k[i] = op(T_{k-1}[i],
    T_{k-1}[i + 2^(k-1)]) with reads past the end giving the identity; a frame
    of L cells at lo, k = floor(log2 L): op(T_k[lo], T_k[hi - 2^k + 1]) is the
    frame's min / max, for every L in 1..130 and an unsegmented table over
    several partitions"""
    op, ident = (min, I64_MAX) if name == "min" else (max, I64_MIN)
    r = np.random.default_rng(22)
    vals, present = random_partition(r, 150, nulls)
    n = len(vals)
    T = [v if p else ident for v, p in zip(vals, present)]
    levels = [T]
    while (1 << len(levels)) <= 130:
        half, prev = 1 << (len(levels) - 1), levels[-1]
        levels.append([op(prev[i], prev[i + half] if i + half < n else ident) for i in range(n)])
    for L in range(1, 131):
        k = L.bit_length() - 1
        for lo in (0, 1, 7, n - L):
            hi = lo + L - 1
            if hi >= n:
                continue
            cells = [vals[j] for j in range(lo, hi + 1) if present[j]]
            exp = op(cells) if cells else ident
            assert op(levels[k][lo], levels[k][hi - (1 << k) + 1]) == exp, (L, lo)


# --------------------------------------------------------------------------
# saturation: a numpy model of k_win_bounds against unbounded integers
# --------------------------------------------------------------------------
def sat_add(a, b):
    """a + b for a >= 0 as the kernel computes it: INT64_MAX instead of a wrap"""
    a, b = np.int64(a), np.int64(b)
    return np.int64(I64_MAX) if b > np.int64(I64_MAX) - a else a + b


def bounds_model(i, ps, pe, start, end):
    lo = max(np.int64(ps), sat_add(i, start))
    hi = min(np.int64(pe), sat_add(i, end))
    return (0, -1) if lo > hi else (int(lo), int(hi))


def test_bounds_saturate_and_never_wrap():
    offsets = (0, 1, -1, 2 ** 31, -2 ** 31, 2 ** 62, -2 ** 62, I64_MAX - 1, I64_MIN + 1)
    ps, pe = 3, 10
    with np.errstate(over="raise"):
        for start in offsets + (UNB_P,):
            for end in offsets + (UNB_F,):
                for i in (ps, 5, pe):
                    lo, hi = frame_of(i - ps, pe - ps + 1, None, ROWS_BETWEEN, start, end)
                    exp = (0, -1) if lo > hi else (lo + ps, hi + ps)
                    assert bounds_model(i, ps, pe, start, end) == exp, (start, end, i)
    # lag / lead / nth_value: i - k cannot wrap for k >= 0; i + k and lo + n - 1 saturate
    assert sat_add(7, 2 ** 62) == 7 + 2 ** 62 and sat_add(7, I64_MAX) == I64_MAX
    assert sat_add(7, I64_MAX - 7) == I64_MAX and sat_add(0, I64_MAX - 1) == I64_MAX - 1


def test_level_count():
    """launches of the level kernel: floor(log2(min(width, n))) + 1, and one
    for a frame that is always empty"""
    def levels(start, end, n):
        if end < start:
            return 1
        return min(end - start + 1, n).bit_length()
    assert levels(-6, 0, 1 << 24) == 3
    assert levels(-1000, 1000, 1 << 24) == 11
    assert levels(0, 0, 5) == 1 and levels(3, 1, 5) == 1
    assert levels(-63, 0, 1 << 20) == 7 and levels(-62, 0, 1 << 20) == 6
    assert levels(-2 ** 62, 2 ** 62, 1025) == 11


# --------------------------------------------------------------------------
# constants
# --------------------------------------------------------------------------
def test_ops_constants_match_the_header():
    import ctypes
    header = open(os.path.join(_ROOT, "include", "trino_gpu.h")).read()
    from trino_amd import ops
    for name, val in (("LAG", LAG), ("LEAD", LEAD), ("FIRST_VALUE", FIRST_VALUE),
                      ("LAST_VALUE", LAST_VALUE), ("NTH_VALUE", NTH_VALUE),
                      ("FRAME_ROWS_BETWEEN", ROWS_BETWEEN)):
        m = re.search(rf"TG_WIN_{name} = (\d+)", header)
        assert m and int(m.group(1)) == val == getattr(ops, f"WIN_{name}"), name
    assert re.search(r"#define TG_WIN_UNBOUNDED_PRECEDING INT64_MIN\b", header)
    assert re.search(r"#define TG_WIN_UNBOUNDED_FOLLOWING INT64_MAX\b", header)
    assert ops.WIN_UNBOUNDED_PRECEDING == UNB_P == -2 ** 63
    assert ops.WIN_UNBOUNDED_FOLLOWING == UNB_F == 2 ** 63 - 1
    assert ctypes.sizeof(ops.TgWindowSpecEx) == 40
    assert ctypes.sizeof(ops.TgWindowSpec) == 16
    assert ops.TgWindowSpecEx.frame_start.offset == 16 and ops.TgWindowSpecEx.offset.offset == 32
