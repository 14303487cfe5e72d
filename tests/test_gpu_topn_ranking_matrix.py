"""TopNRanking operator parity matrix (TopNRankingOp in
trino_amd/csrc/ops_window.hip through trino_amd.ops.topn_ranking), bit-exact
against ref_topn_ranking of tests/test_topn_ranking_reference.py (plain Python
up to PLAIN_ROWS rows, its numpy twin above).

Every case carries a unique BIGINT row-id payload channel (the last input
channel) and asserts
  (1) the kept rows and their order equal the reference's (whole-key ties keep
      input order, so both are fully determined),
  (2) every payload cell and validity bit equals its input row's, with a
      bitmap present exactly where the input channel has one,
  (3) with emit_ranking the last channel is BIGINT without a bitmap and holds
      the reference's rankings; without it the channel is absent, and
  (4) at least one row per partition is kept (m = 0 cannot happen).
Every NULL cell carries a poison value.

The shapes are built in SORTED position space and shuffled, as in
tests/test_gpu_window_matrix.py, so that the kept rows land on chosen lanes,
64-row groups and WSCAN_CHUNK chunks of the rank cut.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from test_gpu_filter_matrix import (Col, KINDS, _NP, POISON, expect_error, make_page, rows_of,
                                    tg_type, unpack_bits, TG_ERR_INVALID_ARG,
                                    TG_ERR_UNSUPPORTED)
from test_gpu_ordering_matrix import canon_key, key_col, page_sizes, slice_cols, special_cols
from test_gpu_window_matrix import layout
from test_topn_ranking_reference import (DENSE_RANK, FN_NAMES, FNS, RANK, ROW_NUMBER, TABLES,
                                         ref_topn_ranking, ref_topn_ranking_vec)
from test_window_reference import RANGE, table_cols

pytestmark = pytest.mark.gpu

TG_ERR_STATE = 4

# assumed by the shapes; test_topn_ranking_reference pins them to the parsed value
C = 1024
EDGE_SIZES = (1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1)
WAVE_CARRIES_ROWS = 64 * C + 1          # the count scan gets one more carry than a wave holds
PLAIN_ROWS = 3000
ENV = "TG_TOPNR_COMPACT_ROWS"


@pytest.fixture(scope="module")
def sess():
    import trino_amd
    s = trino_amd.Session(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ops():
    from trino_amd import ops
    return ops


@contextlib.contextmanager
def compact_rows(rows):
    """TG_TOPNR_COMPACT_ROWS for the operators created inside (the library
    reads it at create); None leaves the environment alone"""
    if rows is None:
        yield
        return
    old = os.environ.get(ENV)
    os.environ[ENV] = str(rows)
    try:
        yield
    finally:
        if old is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = old


# --------------------------------------------------------------------------
# runner
# --------------------------------------------------------------------------
def feed(ops, op, cols, sizes):
    at = 0
    for n in sizes:
        op.add_input(make_page(ops, slice_cols(cols, at, at + n)))
        at += n
    assert at == len(cols[0])


def run_topnr(sess, ops, cols, part, sort, desc, fn, N, emit, sizes, threshold=None):
    with compact_rows(threshold):
        op = ops.topn_ranking(sess, [tg_type(ops, c.kind) for c in cols], part, sort, desc, fn,
                              N, emit)
    try:
        feed(ops, op, cols, sizes)
        pages = op.drain()
    finally:
        op.close()
    return pages


def reference(cols, part, sort, desc, fn, N, emit, plain=None):
    n = len(cols[0])
    if plain is None:
        plain = n <= PLAIN_ROWS
    if plain:
        order, ranking = ref_topn_ranking(rows_of(cols), part, sort, desc, fn, N, emit)
        return (np.array(order, np.int64),
                None if ranking is None else np.array(ranking, np.int64))
    return ref_topn_ranking_vec(cols, part, sort, desc, fn, N, emit)


def assert_page(ops, out, cols, exp, emit, what):
    """one output page against (order, ranking) of a reference"""
    order, ranking = exp
    m = len(order)
    assert len(out) == len(cols) + (1 if emit else 0), f"{what}: {len(out)} channels"
    rid = np.asarray(out[len(cols) - 1]["values"], np.int64)
    assert len(rid) == m, f"{what}: kept {len(rid)} rows, expected {m}"
    assert out[len(cols) - 1]["valid"] is None
    bad = np.flatnonzero(rid != order)
    assert len(bad) == 0, (f"{what}: output row {bad[0]} is input row {rid[bad[0]]}, "
                           f"expected {order[bad[0]]}")
    for c, src in enumerate(cols):
        assert out[c]["type"] == tg_type(ops, src.kind), (what, c, out[c]["type"])
        assert (out[c]["valid"] is None) == (src.valid is None), f"{what}: channel {c} bitmap"
        g = np.asarray(out[c]["values"])
        assert len(g) == m
        gvalid = unpack_bits(out[c]["valid"], m)
        svalid = np.ones(len(src.values), bool) if src.valid is None else src.valid
        assert np.array_equal(gvalid, svalid[rid]), f"{what}: channel {c} validity"
        view = np.int64 if src.kind == "f64" else _NP[src.kind]
        bad = np.flatnonzero((g.view(view) != src.values[rid].view(view)) & gvalid)
        assert len(bad) == 0, f"{what}: channel {c}, output row {bad[0]}"
    if emit:
        o = out[len(cols)]
        assert o["type"] == ops.TG_BIGINT and o["valid"] is None, f"{what}: ranking channel"
        got = np.asarray(o["values"], np.int64)
        bad = np.flatnonzero(got != ranking)
        assert len(bad) == 0, (f"{what}: ranking of output row {bad[0]} is {got[bad[0]]}, "
                               f"expected {ranking[bad[0]]}")


def count_partitions(cols, part):
    keys = list(zip(*[c.cells() for c in (cols[p] for p in part)])) if part else []
    return len({canon_key(k) for k in keys}) if part else 1


def check_topnr(sess, ops, cols, part, sort, desc, fn, N, emit=True, sizes=None, plain=None,
                threshold=None):
    """cols: the LAST column is the unique BIGINT row id. Returns m."""
    n = len(cols[0])
    sizes = page_sizes(n) if sizes is None else sizes
    pages = run_topnr(sess, ops, cols, part, sort, desc, fn, N, emit, sizes, threshold)
    if n == 0:
        assert pages == []
        return 0
    what = f"n={n} {FN_NAMES[fn]} N={N} emit={int(emit)}"
    assert len(pages) == 1, f"{what}: {len(pages)} pages"
    exp = reference(cols, part, sort, desc, fn, N, emit, plain)
    assert_page(ops, pages[0], cols, exp, emit, what)
    m = len(exp[0])
    if n <= PLAIN_ROWS:
        assert m >= count_partitions(cols, part) >= 1, what
    return m


# --------------------------------------------------------------------------
# shapes in sorted-position space
# --------------------------------------------------------------------------
LAYOUTS = ("one", "each", "p64", "straddle", "peer_straddle")


def shape(name, n):
    """(partition id, sort key) per SORTED position, both non-decreasing"""
    pos = np.arange(n, dtype=np.int64)
    if name == "straddle":          # partitions of 100 rows across 64-row and chunk edges
        return (pos + 30) // 100, pos // 3
    pid, skey, _ = layout(name, n)
    return pid, skey


def shape_cols(pid, skey, seed, sort_desc=0):
    """[partition key i64, sort key i32, f64 payload nullable, i16 payload
    nullable, row id], shuffled out of sorted order"""
    n = len(pid)
    r = np.random.default_rng(seed)
    if sort_desc and n:
        skey = skey.max() - skey
    fpresent = r.random(n) >= 0.2
    f = r.standard_normal(n)
    f[~fpresent] = POISON["f64"]
    ypresent = r.random(n) >= 0.5
    y = r.integers(-300, 300, n)
    y[~ypresent] = POISON["i16"]
    shuffle = r.permutation(n)
    cols = [Col("i64", pid * 3 - 7), Col("i32", skey), Col("f64", f, fpresent),
            Col("i16", y, ypresent)]
    cols = [Col(c.kind, c.values[shuffle], None if c.valid is None else c.valid[shuffle])
            for c in cols]
    return cols + [Col("i64", np.arange(n))]


def layout_cols(name, n, seed):
    return shape_cols(*shape(name, n), seed)


@pytest.mark.parametrize("n", EDGE_SIZES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_layouts_every_function_limit_and_emit(sess, ops, name, n):
    cols = layout_cols(name, n, 2000 + n)
    for fn in FNS:
        for N in (1, 2, 63, 64, 65, n + 1):
            for emit in (True, False):
                check_topnr(sess, ops, cols, [0], [1], [0], fn, N, emit)


def test_one_more_count_carry_than_a_wave(sess, ops):
    """64 * WSCAN_CHUNK + 1 rows: 65 chunk counts, two 64-entry groups in the
    one-wave scan of the counts"""
    n = WAVE_CARRIES_ROWS
    pos = np.arange(n, dtype=np.int64)
    # partitions of 100 up to the middle, then one partition to the end with
    # peer groups of 1..C+5 rows, and the last row alone
    pid = np.where(pos < n // 2, pos // 100, n)
    pid[-1] += 1
    skey = np.where(pos % (4 * C) < C + 5, pos // (4 * C) * (4 * C), pos)
    cols = shape_cols(pid, skey, 11)
    for fn in FNS:
        check_topnr(sess, ops, cols, [0], [1], [0], fn, 65, True)
    check_topnr(sess, ops, cols, [0], [1], [0], ROW_NUMBER, 3, False)


# --------------------------------------------------------------------------
# where the cut can go wrong
# --------------------------------------------------------------------------
def kept_positions(cols, part, sort, desc, fn, N):
    """sorted positions of the kept rows, from the reference"""
    from test_window_reference import ref_window
    _, (col,) = ref_window(rows_of(cols), part, sort, desc, [(fn, -1, RANGE)])
    return np.flatnonzero(np.array(col) <= N)


def test_cut_nothing_kept_in_whole_chunks(sess, ops):
    n = 3 * C + 5
    cols = layout_cols("one", n, 81)
    kept = kept_positions(cols, [0], [1], [0], ROW_NUMBER, 5)
    assert kept.max() < C                      # chunks 1.. keep nothing
    for emit in (True, False):
        assert check_topnr(sess, ops, cols, [0], [1], [0], ROW_NUMBER, 5, emit) == 5
    # a kept chunk after two empty ones: the last partition starts in chunk 3
    pos = np.arange(n)
    cols = shape_cols((pos >= 3 * C + 1).astype(np.int64), pos, 82)
    kept = kept_positions(cols, [0], [1], [0], RANK, 2)
    assert kept.tolist() == [0, 1, 3 * C + 1, 3 * C + 2]
    check_topnr(sess, ops, cols, [0], [1], [0], RANK, 2)


@pytest.mark.parametrize("fn", FNS, ids=FN_NAMES)
def test_cut_everything_kept(sess, ops, fn):
    n = 2 * C + 1
    cols = layout_cols("straddle", n, 83)
    for emit in (True, False):
        assert check_topnr(sess, ops, cols, [0], [1], [0], fn, n + 1, emit) == n


def test_cut_keeps_only_in_lane_0_or_lane_63(sess, ops):
    n = 2 * C + 64
    pos = np.arange(n)
    cols = shape_cols(pos // 64, pos, 84)                 # partitions start on lane 0
    kept = kept_positions(cols, [0], [1], [0], ROW_NUMBER, 1)
    assert (kept % 64 == 0).all() and len(kept) == n // 64
    check_topnr(sess, ops, cols, [0], [1], [0], ROW_NUMBER, 1)
    cols = shape_cols((pos + 1) // 64, pos, 85)           # partitions start on lane 63
    kept = kept_positions(cols, [0], [1], [0], ROW_NUMBER, 1)
    assert (kept[1:] % 64 == 63).all() and kept[0] == 0
    for emit in (True, False):
        check_topnr(sess, ops, cols, [0], [1], [0], ROW_NUMBER, 1, emit)


def test_cut_in_the_last_partial_group(sess, ops):
    n = C + 70                                            # the last group holds 6 rows
    pos = np.arange(n)
    cols = shape_cols((pos >= n - 3).astype(np.int64), pos // 2, 86)
    for fn, exp in ((ROW_NUMBER, [0, 1, n - 3, n - 2]), (DENSE_RANK, [0, 1, 2, 3, n - 3, n - 2, n - 1])):
        assert kept_positions(cols, [0], [1], [0], fn, 2).tolist() == exp
        check_topnr(sess, ops, cols, [0], [1], [0], fn, 2)


@pytest.mark.parametrize("fn", FNS, ids=FN_NAMES)
def test_every_partition_keeps_at_least_one_row(sess, ops, fn):
    """m = 0 cannot happen with N >= 1: m >= the number of partitions"""
    n = C + 1
    cols = layout_cols("each", n, 87)
    assert check_topnr(sess, ops, cols, [0], [1], [0], fn, 1) == n
    cols = layout_cols("p64", n, 88)
    assert check_topnr(sess, ops, cols, [0], [1], [0], fn, 1) >= -(-n // 64)


# --------------------------------------------------------------------------
# several pages, compaction forced after every other page
# --------------------------------------------------------------------------
def paged_cols(n, seed, partitions=4, distinct=6):
    """few partitions and few sort keys: ties across pages everywhere"""
    r = np.random.default_rng(seed)
    pkey = Col("i64", r.integers(0, partitions, n), r.random(n) >= 0.1)
    skey = Col("i32", r.integers(0, distinct, n), r.random(n) >= 0.1)
    return [pkey, skey, Col("f64", r.standard_normal(n), r.random(n) >= 0.3),
            Col("i64", np.arange(n))]


PAGED_SIZES = (100,) * 20 + (0,) + (100,) * 20            # a zero-row page in the middle


@pytest.mark.parametrize("fn", FNS, ids=FN_NAMES)
def test_forty_pages_compacted_as_they_arrive(sess, ops, fn):
    cols = paged_cols(4000, 91)
    for N in (1, 7, 300):
        for emit in (True, False):
            check_topnr(sess, ops, cols, [0], [1], [1], fn, N, emit, sizes=PAGED_SIZES,
                        threshold=128)
    check_topnr(sess, ops, cols, [], [1], [0], fn, 7, True, sizes=PAGED_SIZES, threshold=128)
    check_topnr(sess, ops, cols, [0], [], [], fn, 7, True, sizes=PAGED_SIZES, threshold=128)


def test_row_number_ties_keep_input_order_across_pages(sess, ops):
    cols = paged_cols(4000, 92, partitions=2, distinct=2)
    pages = run_topnr(sess, ops, cols, [0], [1], [0], ROW_NUMBER, 500, True, PAGED_SIZES, 128)
    out = pages[0]
    rid = np.asarray(out[3]["values"], np.int64)
    rows = rows_of(cols)
    keys = [canon_key(rows[i][:2]) for i in rid]
    for a in range(1, len(rid)):
        if keys[a] == keys[a - 1]:
            assert rid[a] > rid[a - 1], f"output rows {a - 1}, {a}: a tie out of input order"
    # and the kept rows of a tied key are its EARLIEST input rows
    exp = reference(cols, [0], [1], [0], ROW_NUMBER, 500, True)
    assert_page(ops, out, cols, exp, True, "ties across pages")


@pytest.mark.parametrize("fn", FNS, ids=FN_NAMES)
def test_nothing_can_be_cut_still_yields_the_full_input(sess, ops, fn):
    """N >= every partition: every compaction retains all it was given, and
    the 2x rule spaces the compactions out; the result is the Window's page"""
    cols = paged_cols(4000, 93)
    assert check_topnr(sess, ops, cols, [0], [1], [0], fn, 4001, True, sizes=PAGED_SIZES,
                       threshold=128) == 4000


@pytest.mark.parametrize("fn", FNS, ids=FN_NAMES)
def test_partial_then_final(sess, ops, fn):
    """two emit_ranking = 0 operators take half of the pages each; their
    outputs, fed in that order to one emit_ranking = 1 operator, give the
    single-operator result"""
    n, N = 4000, 9
    cols = paged_cols(n, 94)
    types = [tg_type(ops, c.kind) for c in cols]
    with compact_rows(128):
        partial = [ops.topn_ranking(sess, types, [0], [1], [1], fn, N, False) for _ in range(2)]
        final = ops.topn_ranking(sess, types, [0], [1], [1], fn, N, True)
    try:
        for h, op in enumerate(partial):
            lo = h * n // 2
            feed(ops, op, slice_cols(cols, lo, lo + n // 2), (100,) * 20)
            (out,) = op.drain()
            assert len(out) == len(cols)
            m = len(out[0]["values"])
            back = [Col(c.kind, o["values"], None if o["valid"] is None
                        else unpack_bits(o["valid"], m)) for c, o in zip(cols, out)]
            final.add_input(make_page(ops, back))
        (got,) = final.drain()
    finally:
        for op in partial + [final]:
            op.close()
    assert_page(ops, got, cols, reference(cols, [0], [1], [1], fn, N, True), True,
                f"partial to final {FN_NAMES[fn]}")


@pytest.mark.parametrize("fn", FNS, ids=FN_NAMES)
def test_equals_window_then_filter_on_device(sess, ops, fn):
    """ops.window with the ranking spec, then ops.filter_project with
    rank <= N, gives the cells of ops.topn_ranking"""
    n, N = C + 77, 5
    cols = layout_cols("straddle", n, 95)
    types = [tg_type(ops, c.kind) for c in cols]
    (mine,) = run_topnr(sess, ops, cols, [0], [1], [0], fn, N, True, page_sizes(n))
    win = ops.window(sess, types, [0], [1], [0], [(fn, -1, ops.WIN_FRAME_RANGE)])
    k = len(cols)
    filt = ops.expr(("col", k), ("i64", N), "le")
    proj = [ops.expr(("col", j)) for j in range(k + 1)]
    fp = ops.filter_project(sess, filt, proj, types + [ops.TG_BIGINT])
    try:
        feed(ops, win, cols, page_sizes(n))
        (wout,) = win.drain()
        wcols = [Col(c.kind, o["values"], None if o["valid"] is None else unpack_bits(o["valid"], n))
                 for c, o in zip(cols + [Col("i64", [])], wout)]
        fp.add_input(make_page(ops, wcols))
        (theirs,) = fp.drain()
    finally:
        win.close()
        fp.close()
    assert len(mine) == len(theirs) == k + 1
    m = len(mine[0]["values"])
    for j, (a, b) in enumerate(zip(mine, theirs)):
        assert a["type"] == b["type"] and len(b["values"]) == m, j
        av, bv = unpack_bits(a["valid"], m), unpack_bits(b["valid"], m)
        assert np.array_equal(av, bv), f"channel {j}: validity"
        view = np.int64 if a["values"].dtype == np.float64 else a["values"].dtype
        assert np.array_equal(a["values"].view(view)[av], b["values"].view(view)[bv]), j


# --------------------------------------------------------------------------
# keys
# --------------------------------------------------------------------------
def payload_and_id(n, seed):
    r = np.random.default_rng(seed)
    null = r.random(n) < 0.3
    x = r.integers(-5000, 5000, n)
    x[null] = POISON["i64"]
    return [Col("i64", x, ~null), Col("i64", np.arange(n))]


@pytest.mark.parametrize("desc", [0, 1], ids=["asc", "desc"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_type_as_partition_and_sort_key(sess, ops, kind, desc):
    n = C + 1
    cols = [key_col(kind, n, 21, 0.1, 0, distinct=9), key_col(kind, n, 22, 0.1, desc, distinct=5)]
    cols += payload_and_id(n, 23)
    for fn in FNS:
        check_topnr(sess, ops, cols, [0], [1], [desc], fn, 3, fn != RANK)


@pytest.mark.parametrize("desc", [[0, 1], [1, 0], [1, 1]], ids=str)
def test_two_partition_and_two_sort_channels(sess, ops, desc):
    n = 2 * C + 1
    cols = [key_col("i32", n, 31, 0.1, 0, distinct=4), key_col("f64", n, 32, 0.1, 0, distinct=3),
            key_col("i64", n, 33, 0.2, desc[0], distinct=5),
            key_col("i16", n, 34, 0.2, desc[1], distinct=4), Col("i64", np.arange(n))]
    for fn in FNS:
        check_topnr(sess, ops, cols, [0, 1], [2, 3], desc, fn, 4)


@pytest.mark.parametrize("desc", [0, 1], ids=["asc", "desc"])
@pytest.mark.parametrize("name", ["int64_extremes", "double_specials", "all_ones_nan"])
def test_special_keys(sess, ops, name, desc):
    """NULL / NaN with either sign / -0.0 / INT64_MIN / INT64_MAX keys, as
    the partition key and as the sort key"""
    n = C + 1
    cols = [special_cols(name, n, 41), special_cols(name, n, 42)] + payload_and_id(n, 43)
    for fn in FNS:
        check_topnr(sess, ops, cols, [0], [1], [desc], fn, 2)


@pytest.mark.parametrize("fn", FNS, ids=FN_NAMES)
def test_no_partition_no_sort_or_neither(sess, ops, fn):
    n, N = C + 1, 70
    cols = [key_col("i16", n, 51, 0.1, 0, distinct=7), key_col("f64", n, 52, 0.1, 1, distinct=40)]
    cols += payload_and_id(n, 53)
    check_topnr(sess, ops, cols, [], [1], [1], fn, N)                 # one partition
    m = check_topnr(sess, ops, cols, [0], [], [], fn, N)              # every row a peer
    if fn != ROW_NUMBER:
        assert m == n                                                 # rank 1 everywhere
    m = check_topnr(sess, ops, cols, [], [], [], fn, N)
    assert m == (N if fn == ROW_NUMBER else n)
    if fn == ROW_NUMBER:                                              # the first N input rows
        (out,) = run_topnr(sess, ops, cols, [], [], [], fn, N, True, page_sizes(n))
        assert out[3]["values"].tolist() == list(range(N))
        assert out[4]["values"].tolist() == list(range(1, N + 1))


def test_empty_input_and_all_empty_pages(sess, ops):
    cols = [key_col("i64", 0, 1, 0, 0), key_col("i64", 0, 2, 0, 0)] + payload_and_id(0, 2)
    for sizes in ((), (0,), (0, 0, 0)):
        for emit in (True, False):
            check_topnr(sess, ops, cols, [0], [1], [0], ROW_NUMBER, 3, emit, sizes=sizes)
    cols = layout_cols("p64", 65, 3)
    check_topnr(sess, ops, cols, [0], [1], [0], RANK, 2, sizes=(0, 64, 0, 1, 0))


@pytest.mark.parametrize("name", sorted(TABLES))
def test_hand_written_tables(sess, ops, name):
    """the typed-out expectations of test_topn_ranking_reference, on the device"""
    t = TABLES[name]
    n = len(t["rows"])
    cols = table_cols(t["rows"]) + [Col("i64", np.arange(n))]
    for fn in FNS:
        (out,) = run_topnr(sess, ops, cols, t["part"], t["sort"], t["desc"], fn, t["N"], True,
                           (n,))
        assert (out[-2]["values"].tolist(), out[-1]["values"].tolist()) == t["out"][fn], fn


# --------------------------------------------------------------------------
# bounded memory
# --------------------------------------------------------------------------
def test_memory_is_bounded_by_the_threshold_not_the_input(sess, ops):
    """one partition, N = 4, threshold 8192, 64 pages of 4096 rows: the live
    bytes cycle (at most threshold + one page + retained rows), so the peak
    over pages 9..64 does not exceed the peak over pages 1..8; the Window
    holds every row"""
    from trino_amd import session_memory

    def live():
        total, cached = session_memory(sess)
        return total - cached

    r = np.random.default_rng(97)
    rows, npages = 4096, 64
    B = ops.TG_BIGINT
    pages = [[Col("i64", np.zeros(rows, np.int64)), Col("i64", r.integers(0, 1 << 40, rows)),
              Col("i64", np.arange(p * rows, (p + 1) * rows))] for p in range(npages)]
    start = live()
    with compact_rows(8192):
        op = ops.topn_ranking(sess, [B] * 3, [0], [1], [0], ROW_NUMBER, 4, True)
    seen = []
    try:
        for cols in pages:
            op.add_input(make_page(ops, cols))
            seen.append(live() - start)
        (out,) = op.drain()
    finally:
        op.close()
    assert live() == start
    print("live bytes after each add_input:", seen)
    assert max(seen[8:]) <= max(seen[:8]), (max(seen[8:]), max(seen[:8]))
    allc = [Col("i64", np.concatenate([p[c].values for p in pages])) for c in range(3)]
    assert_page(ops, out, allc, reference(allc, [0], [1], [0], ROW_NUMBER, 4, True, plain=False),
                True, "bounded memory")
    win = ops.window(sess, [B] * 3, [0], [1], [0], [(ROW_NUMBER, -1, ops.WIN_FRAME_RANGE)])
    try:
        for cols in pages:
            win.add_input(make_page(ops, cols))
        held = live() - start
    finally:
        win.close()
    print("the Window's live bytes after page 64:", held)
    assert held > seen[-1] and held > max(seen)


# --------------------------------------------------------------------------
# ABI behaviour
# --------------------------------------------------------------------------
def raw_create(ops, sess, types, part, n_part, sort, sort_desc, n_sort, fn=0, N=1, emit=1,
               null_session=False, null_types=False, null_out=False):
    """tg_topn_ranking_create with every pointer and count under the caller's control"""
    from trino_amd import _lib, _check
    ty = np.array(types, np.int32)
    arr = lambda v: None if v is None else np.array(v, np.int32)      # noqa: E731
    pc, sc, sd = arr(part), arr(sort), arr(sort_desc)
    h = ctypes.c_void_p()
    ptr = lambda a: None if a is None else a.ctypes.data              # noqa: E731
    st = _lib.tg_topn_ranking_create(None if null_session else sess._h,
                                     None if null_types else ty.ctypes.data, len(ty),
                                     ptr(pc), n_part, ptr(sc), ptr(sd), n_sort, fn, N, emit,
                                     None if null_out else ctypes.byref(h))
    assert (st == 0) == bool(h.value)
    if h.value:
        _lib.tg_operator_close(h)
    _check(st)


def test_rejections_by_status(sess, ops):
    B, D, V = ops.TG_BIGINT, ops.TG_DOUBLE, ops.TG_VARCHAR
    ok = dict(types=[B, B], part=[0], n_part=1, sort=[1], sort_desc=[0], n_sort=1)
    raw_create(ops, sess, **ok)                                   # the base case is accepted
    inv = lambda **kw: expect_error(lambda: raw_create(ops, sess, **{**ok, **kw}),   # noqa: E731
                                    TG_ERR_INVALID_ARG)
    inv(null_session=True)
    inv(null_types=True)
    inv(null_out=True)
    inv(part=None)                      # null arrays with a non-zero count
    inv(sort=None)
    inv(sort_desc=None)
    for ch in (-1, 2, 7):
        inv(part=[ch])
        inv(sort=[ch])
    for fn in (-1, 3, 12):
        inv(fn=fn)
    for N in (0, -1, -2 ** 31):
        inv(N=N)
    for emit in (-1, 2):
        inv(emit=emit)
    uns = lambda word, **kw: expect_error(lambda: raw_create(ops, sess, **{**ok, **kw}),  # noqa: E731
                                          TG_ERR_UNSUPPORTED, word)
    uns("VARCHAR", types=[B, V], sort=[0])
    uns("VARCHAR", types=[V, B], part=[1])
    uns("VARCHAR", types=[B, B, V])
    # DOUBLE keys, zero counts with null arrays, every function, emit 0, a large N
    raw_create(ops, sess, **{**ok, "types": [D, D]})
    raw_create(ops, sess, **{**ok, "part": None, "n_part": 0, "sort": None, "sort_desc": None,
                             "n_sort": 0})
    for fn in FNS:
        raw_create(ops, sess, **ok, fn=fn, emit=0, N=2 ** 31 - 1)


def test_add_input_rejections_and_state_machine(sess, ops):
    B = ops.TG_BIGINT
    op = ops.topn_ranking(sess, [B, B], [0], [1], [0], ROW_NUMBER, 1)
    try:
        narrow = [Col("i64", [1, 2]), Col("i32", [1, 2])]
        expect_error(lambda: op.add_input(make_page(ops, narrow)), TG_ERR_INVALID_ARG,
                     "topn_ranking")
        expect_error(lambda: op.add_input(make_page(ops, narrow[:1])), TG_ERR_INVALID_ARG,
                     "topn_ranking")
        good = [Col("i64", [2, 1, 2]), Col("i64", [5, 6, 4])]
        op.add_input(make_page(ops, good))
        assert op.get_output() == (None, False)          # before finish: no page
        op.finish()
        expect_error(lambda: op.add_input(make_page(ops, good)), TG_ERR_STATE)
        cols, fin = op.get_output()
        assert not fin and cols[0]["values"].tolist() == [1, 2]
        assert cols[1]["values"].tolist() == [6, 4] and cols[2]["values"].tolist() == [1, 1]
        assert op.get_output() == (None, True)
        assert op.get_output() == (None, True)
    finally:
        op.close()


def test_memory_returns_after_close(sess, ops):
    """live pool bytes (total - cached) after close equal the starting value:
    with output fetched, with output staged but not fetched, closed without
    finish (a retained page and a staged page held), and after a rejected page"""
    from trino_amd import session_memory

    def live():
        total, cached = session_memory(sess)
        return total - cached

    cols = layout_cols("p64", 2 * C + 1, 71)
    types = [tg_type(ops, c.kind) for c in cols]
    start = live()
    for mode in ("drained", "staged", "unfinished", "rejected_page"):
        with compact_rows(2 * C):
            op = ops.topn_ranking(sess, types, [0], [1], [0], RANK, 2, True)
        op.add_input(make_page(ops, cols))               # compacted at once
        op.add_input(make_page(ops, slice_cols(cols, 0, 100)))
        assert live() > start
        if mode == "drained":
            assert len(op.drain()) == 1
        elif mode == "staged":                 # the output page stays with the operator
            op.finish()
            assert op.get_output()[0] is not None
        elif mode == "rejected_page":
            expect_error(lambda: op.add_input(make_page(ops, cols[:2])), TG_ERR_INVALID_ARG)
        op.close()
        assert live() == start, mode
