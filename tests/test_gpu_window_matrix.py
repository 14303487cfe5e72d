"""Window operator parity matrix (trino_amd/csrc/ops_window.hip through
trino_amd.ops.window), bit-exact against the references of
tests/test_window_reference.py: ref_window (plain Python) up to PLAIN_ROWS
rows, its numpy twin ref_window_vec above.

Every case carries a unique BIGINT row-id payload channel (the last input
channel) and asserts
  (1) the output row order equals the reference's (whole-key ties keep input
      order, so the order is fully determined),
  (2) every payload cell and validity bit equals its input row's,
  (3) every spec column equals the reference's values, and
  (4) its validity equals the reference's, with a bitmap present exactly for
      SUM / MIN / MAX.
Every NULL cell carries a poison value.

The shapes are built in SORTED position space (which partition and which peer
group each sorted position belongs to, where the non-NULL inputs lie) and then
shuffled, so partition and peer boundaries land on chosen offsets of the
segmented scan: 64-row group edges, WSCAN_CHUNK edges, chunks without a head.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_filter_matrix import (Col, KINDS, _NP, POISON, expect_error, make_page, rows_of,
                                    tg_type, unpack_bits, TG_ERR_INVALID_ARG,
                                    TG_ERR_UNSUPPORTED)
from test_gpu_ordering_matrix import key_col, page_sizes, slice_cols, special_cols
from test_window_reference import (ALL_SPECS, COUNT_COL, COUNT_STAR, DENSE_RANK, I64_MAX,
                                   I64_MIN, MAX_I64, MIN_I64, PARTITION, RANGE, RANK,
                                   ROW_NUMBER, ROWS, SUM_I64, TABLES, as_arrays, assert_same,
                                   has_validity, ref_window, ref_window_vec, table_cols)

pytestmark = pytest.mark.gpu

TG_ERR_STATE = 4

# assumed by the shapes; test_window_reference pins them to the parsed values
WSCAN_CHUNK = 1024
WSCAN_ONE_WAVE = 1024
C = WSCAN_CHUNK
EDGE_SIZES = (1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1)
WAVE_CARRIES_ROWS = 64 * C + 1                  # one more carry than a wave holds
DEEP_ROWS = WSCAN_CHUNK * WSCAN_ONE_WAVE + 1    # the carry scan recurses
PLAIN_ROWS = 3000                               # ref_window up to here, ref_window_vec above


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


# --------------------------------------------------------------------------
# runner
# --------------------------------------------------------------------------
def run_window(sess, ops, cols, part, sort, desc, specs, sizes):
    op = ops.window(sess, [tg_type(ops, c.kind) for c in cols], part, sort, desc, specs)
    try:
        at = 0
        for n in sizes:
            op.add_input(make_page(ops, slice_cols(cols, at, at + n)))
            at += n
        assert at == len(cols[0])
        pages = op.drain()
    finally:
        op.close()
    return pages


def check_window(sess, ops, cols, part, sort, desc, specs, sizes=None, plain=None):
    """cols: the LAST column is the unique BIGINT row id"""
    n = len(cols[0])
    sizes = page_sizes(n) if sizes is None else sizes
    pages = run_window(sess, ops, cols, part, sort, desc, specs, sizes)
    if n == 0:
        assert pages == []
        return
    assert len(pages) == 1 and len(pages[0]) == len(cols) + len(specs)
    out = pages[0]
    if plain is None:
        plain = n <= PLAIN_ROWS
    if plain:
        order, ref_cols = ref_window(rows_of(cols), part, sort, desc, specs)
        exp = (np.array(order, np.int64), as_arrays(ref_cols, specs))
    else:
        exp = ref_window_vec(cols, part, sort, desc, specs)
    # (1) the row order, through the row id
    rid = np.asarray(out[len(cols) - 1]["values"], np.int64)
    assert len(rid) == n and out[len(cols) - 1]["valid"] is None
    bad = np.flatnonzero(rid != exp[0])
    assert len(bad) == 0, f"output row {bad[0]} is input row {rid[bad[0]]}, expected {exp[0][bad[0]]}"
    # (2) the payload: every channel of every row, validity included
    for c, src in enumerate(cols):
        assert out[c]["type"] == tg_type(ops, src.kind), (c, out[c]["type"])
        assert (out[c]["valid"] is None) == (src.valid is None), f"channel {c}: bitmap presence"
        g = np.asarray(out[c]["values"])
        gvalid = unpack_bits(out[c]["valid"], n)
        svalid = np.ones(n, bool) if src.valid is None else src.valid
        assert np.array_equal(gvalid, svalid[rid]), f"channel {c}: validity"
        view = np.int64 if src.kind == "f64" else _NP[src.kind]
        bad = np.flatnonzero((g.view(view) != src.values[rid].view(view)) & gvalid)
        assert len(bad) == 0, f"channel {c}: output row {bad[0]} is not input row {rid[bad[0]]}"
    # (3), (4) the spec columns
    got = []
    for k, (fn, _, _) in enumerate(specs):
        o = out[len(cols) + k]
        assert o["type"] == ops.TG_BIGINT
        assert (o["valid"] is not None) == has_validity(fn), f"spec {k}: bitmap presence"
        got.append((np.asarray(o["values"], np.int64),
                    None if o["valid"] is None else unpack_bits(o["valid"], n)))
    assert_same((rid, got), exp, specs, f"n={n}")


# --------------------------------------------------------------------------
# shapes in sorted-position space
# --------------------------------------------------------------------------
LAYOUTS = ("one", "each", "pairs", "p64", "edges", "long", "peer_straddle", "late_nonnull",
           "last_alone")


def layout(name, n):
    """(partition id, sort key, input-present mask) per SORTED position; ids
    and keys are non-decreasing so that sorting reproduces the positions"""
    pos = np.arange(n, dtype=np.int64)
    pid = np.zeros(n, np.int64)
    skey = pos // 3                      # peer groups of 3 by default
    present = None
    if name == "one":
        pass
    elif name == "each":                 # every row its own partition
        pid = pos.copy()
    elif name == "pairs":
        pid = pos // 2
    elif name == "p64":                  # every boundary on a 64-row edge
        pid = pos // 64
    elif name == "edges":                # boundaries exactly at 64, C and 2C
        pid = (pos >= 64).astype(np.int64) + (pos >= C) + (pos >= 2 * C)
    elif name == "long":
        # a short partition, then one that runs to the end: with n > 2C it
        # covers whole chunks that hold no head, and a carry passes through
        pid = (pos >= 5).astype(np.int64)
        skey = pos // 700                # peer groups longer than half a chunk
    elif name == "peer_straddle":        # one peer group over the chunk edge
        lo, hi = max(C - 2, 0), C + 3
        skey = np.where(pos < lo, pos // 2, np.where(pos < hi, lo, hi + pos // 5))
    elif name == "late_nonnull":
        # partition 1 starts 10 rows before the chunk edge and its non-NULL
        # inputs all lie after it: its validity can only come from the carry;
        # partition 0 before it is full of non-NULLs the reset must drop
        start = max(min(C, n) - 10, 0)
        pid = (pos >= start).astype(np.int64)
        present = (pos < start) | (pos >= C + 3)
    elif name == "last_alone":           # the last row alone in its partition
        pid = pos // 7
        pid[-1] = pid[-1] + 1 if n > 1 and pid[-1] == pid[-2] else pid[-1]
    else:
        raise ValueError(name)
    return pid, skey, present


def layout_cols(name, n, seed, sort_desc=0):
    """[partition key i64, sort key i32, x i64 nullable, y i16 nullable,
    f64 payload nullable, row id], shuffled out of sorted order"""
    r = np.random.default_rng(seed)
    pid, skey, present = layout(name, n)
    if sort_desc:
        skey = skey.max() - skey if n else skey
    if present is None:
        present = r.random(n) >= 0.3
    x = r.integers(-1000, 1000, n)
    x[~present] = POISON["i64"]
    ypresent = r.random(n) >= 0.5
    y = r.integers(-300, 300, n)
    y[~ypresent] = POISON["i16"]
    fpresent = r.random(n) >= 0.2
    shuffle = r.permutation(n)
    cols = [Col("i64", pid * 3 - 7), Col("i32", skey), Col("i64", x, present),
            Col("i16", y, ypresent), Col("f64", r.standard_normal(n), fpresent)]
    cols = [Col(c.kind, c.values[shuffle], None if c.valid is None else c.valid[shuffle])
            for c in cols]
    return cols + [Col("i64", np.arange(n))]


# every function x frame, eight specs per operator (the ABI's limit)
SPEC_GROUPS = (ALL_SPECS[:8], ALL_SPECS[8:16],
               ALL_SPECS[16:] + [(SUM_I64, 3, RANGE), (MIN_I64, 3, ROWS), (MAX_I64, 3, PARTITION),
                                 (COUNT_COL, 3, RANGE), (RANK, -1, RANGE), (SUM_I64, 2, ROWS)])


def test_spec_groups_cover_every_function_and_frame():
    assert all(len(g) == 8 for g in SPEC_GROUPS)
    seen = {(fn, fr) for g in SPEC_GROUPS for fn, _, fr in g}
    assert {(fn, RANGE) for fn in (ROW_NUMBER, RANK, DENSE_RANK)} <= seen
    assert {(fn, fr) for fn in (COUNT_STAR, COUNT_COL, SUM_I64, MIN_I64, MAX_I64)
            for fr in (RANGE, ROWS, PARTITION)} <= seen


@pytest.mark.parametrize("n", EDGE_SIZES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_layouts_every_function_and_frame(sess, ops, name, n):
    cols = layout_cols(name, n, 1000 + n)
    for specs in SPEC_GROUPS:
        check_window(sess, ops, cols, [0], [1], [0], specs)


@pytest.mark.parametrize("name", ["long", "peer_straddle", "late_nonnull"])
def test_layouts_descending_sort(sess, ops, name):
    cols = layout_cols(name, 2 * C + 1, 7, sort_desc=1)
    check_window(sess, ops, cols, [0], [1], [1], SPEC_GROUPS[1])


def big_cols(n, seed):
    """a short partition, one over 3 chunks and 7 rows, partitions of 64 up
    to the middle, then one partition across everything after it (it crosses
    the edge between the chunks of CARRIES when those are scanned in three
    launches) and the last row alone; peer groups of 1..C+5 rows"""
    r = np.random.default_rng(seed)
    pos = np.arange(n, dtype=np.int64)
    a, b, mid = 5, 5 + 3 * C + 7, n // 2
    pid = np.where(pos < a, 0, np.where(pos < b, 1, np.where(pos < mid, 2 + pos // 64,
                                                           2 + mid)))
    pid[-1] += 1
    skey = np.where(pos % (4 * C) < C + 5, pos // (4 * C) * (4 * C), pos)
    present = r.random(n) >= 0.3
    present[mid:mid + C + 9] = False            # the long partition starts with NULLs
    x = r.integers(-10 ** 12, 10 ** 12, n)
    x[~present] = POISON["i64"]
    shuffle = r.permutation(n)
    cols = [Col("i64", pid), Col("i64", skey), Col("i64", x, present)]
    cols = [Col(c.kind, c.values[shuffle], None if c.valid is None else c.valid[shuffle])
            for c in cols]
    return cols + [Col("i64", np.arange(n))]


BIG_SPECS = [(ROW_NUMBER, -1, RANGE), (RANK, -1, RANGE), (DENSE_RANK, -1, RANGE),
             (SUM_I64, 2, RANGE), (MIN_I64, 2, ROWS), (MAX_I64, 2, PARTITION),
             (COUNT_COL, 2, ROWS), (COUNT_STAR, -1, RANGE)]


def test_one_more_carry_than_a_wave(sess, ops):
    """64 * WSCAN_CHUNK + 1 rows: 65 carries, two 64-row groups in the
    one-wave carry scan; checked by both references"""
    cols = big_cols(WAVE_CARRIES_ROWS, 11)
    check_window(sess, ops, cols, [0], [1], [0], BIG_SPECS, plain=True)
    check_window(sess, ops, cols, [0], [1], [0], BIG_SPECS, plain=False)


def test_carry_scan_recurses(sess, ops):
    """the smallest input whose carries exceed one wave's threshold: the
    deepest path of run_wscan"""
    cols = big_cols(DEEP_ROWS, 12)
    check_window(sess, ops, cols, [0], [1], [0], BIG_SPECS)


def test_carry_scan_recurses_single_partition(sess, ops):
    """no partition channel at the deepest size: every carry at both levels
    passes through, and the reverse scan's one segment is the whole input"""
    n = DEEP_ROWS
    r = np.random.default_rng(13)
    cols = [Col("i64", r.integers(0, 50, n)), Col("i64", r.integers(-9, 9, n), r.random(n) >= 0.5),
            Col("i64", np.arange(n))]
    check_window(sess, ops, cols, [], [0], [0],
                 [(ROW_NUMBER, -1, RANGE), (RANK, -1, RANGE), (SUM_I64, 1, RANGE),
                  (MIN_I64, 1, PARTITION)])


# --------------------------------------------------------------------------
# keys
# --------------------------------------------------------------------------
KEY_SPECS = [(ROW_NUMBER, -1, RANGE), (RANK, -1, RANGE), (DENSE_RANK, -1, RANGE),
             (SUM_I64, 2, RANGE), (COUNT_COL, 2, PARTITION)]


def input_and_id(n, seed):
    r = np.random.default_rng(seed)
    null = r.random(n) < 0.3
    x = r.integers(-5000, 5000, n)
    x[null] = POISON["i64"]
    return [Col("i64", x, ~null), Col("i64", np.arange(n))]


@pytest.mark.parametrize("desc", [0, 1], ids=["asc", "desc"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_type_as_partition_and_sort_key(sess, ops, kind, desc):
    """the same type as partition key (always ASC NULLS LAST) and as sort key
    in both directions; 10 % NULL keys over the value that would sort first"""
    n = C + 1
    cols = [key_col(kind, n, 21, 0.1, 0, distinct=9), key_col(kind, n, 22, 0.1, desc, distinct=5)]
    cols += input_and_id(n, 23)
    check_window(sess, ops, cols, [0], [1], [desc], KEY_SPECS)


@pytest.mark.parametrize("desc", [[0, 1], [1, 0], [1, 1]], ids=str)
def test_two_partition_and_two_sort_channels(sess, ops, desc):
    n = 2 * C + 1
    cols = [key_col("i32", n, 31, 0.1, 0, distinct=4), key_col("f64", n, 32, 0.1, 0, distinct=3),
            key_col("i64", n, 33, 0.2, desc[0], distinct=5),
            key_col("i16", n, 34, 0.2, desc[1], distinct=4)]
    # channel 2 is both a sort key and the aggregate input
    cols[2] = Col("i64", np.where(cols[2].valid, cols[2].values % 1000, POISON["i64"]),
                  cols[2].valid)
    cols += [Col("i64", np.arange(n))]
    check_window(sess, ops, cols, [0, 1], [2, 3], desc, KEY_SPECS)


@pytest.mark.parametrize("desc", [0, 1], ids=["asc", "desc"])
@pytest.mark.parametrize("name", ["int64_extremes", "double_specials", "all_ones_nan"])
def test_special_keys(sess, ops, name, desc):
    """NULL / NaN (five bit patterns) / -0.0 / INT64_MIN / INT64_MAX keys, as
    the partition key and as the sort key"""
    n = C + 1
    cols = [special_cols(name, n, 41), special_cols(name, n, 42)] + input_and_id(n, 43)
    check_window(sess, ops, cols, [0], [1], [desc], KEY_SPECS)


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
AGG_SPECS = [(fn, 1, fr) for fn in (SUM_I64, MIN_I64, MAX_I64, COUNT_COL) for fr in (ROWS, RANGE)]


@pytest.mark.parametrize("kind", [k for k in KINDS if k != "f64"])
def test_every_integer_width_as_input(sess, ops, kind):
    n = C + 1
    r = np.random.default_rng(51)
    if kind == "bool":
        vals = r.integers(0, 2, n)
    else:
        info = np.iinfo(_NP[kind])
        vals = r.integers(max(info.min, -2 ** 40), min(info.max, 2 ** 40), n, endpoint=True)
        vals[:4] = (info.min, info.max, -1, 0)
    null = r.random(n) < 0.3
    vals = np.asarray(vals, _NP[kind])
    vals[null] = POISON[kind]
    cols = [Col("i32", r.integers(0, 9, n)), Col(kind, vals, ~null),
            Col("i16", r.integers(0, 40, n)), Col("i64", np.arange(n))]
    check_window(sess, ops, cols, [0], [2], [0], AGG_SPECS)


def test_min_max_over_int64_extremes_and_negative_sums(sess, ops):
    n = 2 * C + 1
    r = np.random.default_rng(52)
    pool = np.array([I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1, 0, -1, -10 ** 18], np.int64)
    x = pool[r.integers(0, len(pool), n)]
    null = r.random(n) < 0.4
    x[null] = POISON["i64"]
    neg = -r.integers(1, 10 ** 15, n)
    cols = [Col("i64", r.integers(0, 40, n)), Col("i64", x, ~null), Col("i64", neg),
            Col("i8", r.integers(0, 12, n)), Col("i64", np.arange(n))]
    specs = [(MIN_I64, 1, ROWS), (MAX_I64, 1, ROWS), (MIN_I64, 1, PARTITION),
             (MAX_I64, 1, RANGE), (SUM_I64, 1, ROWS), (SUM_I64, 2, ROWS), (SUM_I64, 2, RANGE),
             (SUM_I64, 2, PARTITION)]
    check_window(sess, ops, cols, [0], [3], [1], specs)


# --------------------------------------------------------------------------
# stability, empty inputs, the hand-written tables
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 2 * C + 1])
def test_all_keys_tie_keeps_input_order(sess, ops, n):
    zeros = np.where(np.arange(n) % 2, -0.0, 0.0)           # -0.0 ties with 0.0
    cols = [Col("i64", np.full(n, 7)), Col("f64", zeros), Col("i64", np.arange(n))]
    specs = [(ROW_NUMBER, -1, RANGE), (RANK, -1, RANGE), (COUNT_STAR, -1, ROWS)]
    for part, sort, desc in (([0], [1], [1]), ([], [0, 1], [0, 1]), ([0, 1], [], [])):
        pages = run_window(sess, ops, cols, part, sort, desc, specs, page_sizes(n))
        out = pages[0]
        assert np.array_equal(out[2]["values"], np.arange(n))
        assert np.array_equal(out[3]["values"], np.arange(n) + 1)
        assert np.array_equal(out[4]["values"], np.ones(n, np.int64))
        check_window(sess, ops, cols, part, sort, desc, specs)


def test_no_channels_runs_no_sort(sess, ops):
    n = C + 1
    cols = input_and_id(n, 61)
    check_window(sess, ops, cols, [], [], [], [(ROW_NUMBER, -1, RANGE), (SUM_I64, 0, ROWS),
                                               (SUM_I64, 0, RANGE), (MAX_I64, 0, PARTITION)])


def test_empty_input_and_all_empty_pages(sess, ops):
    cols = [key_col("i64", 0, 1, 0, 0)] + input_and_id(0, 2)
    for sizes in ((), (0,), (0, 0, 0)):
        check_window(sess, ops, cols, [0], [1], [0], KEY_SPECS[:3], sizes=sizes)
    # an empty page among full ones
    cols = layout_cols("pairs", 65, 3)
    check_window(sess, ops, cols, [0], [1], [0], SPEC_GROUPS[0], sizes=(0, 64, 0, 1, 0))


@pytest.mark.parametrize("name", sorted(TABLES))
def test_hand_written_tables(sess, ops, name):
    """the typed-out expectations of test_window_reference, on the device"""
    t = TABLES[name]
    cols = table_cols(t["rows"])
    n = len(t["rows"])
    cols.append(Col("i64", np.arange(n)))
    pages = run_window(sess, ops, cols, t["part"], t["sort"], t["desc"], t["specs"], (n,))
    out = pages[0]
    assert out[len(cols) - 1]["values"].tolist() == t["order"]
    for k, exp in enumerate(t["cols"]):
        o = out[len(cols) + k]
        valid = unpack_bits(o["valid"], n)
        got = [int(v) if ok else None for v, ok in zip(o["values"].tolist(), valid.tolist())]
        assert got == exp, (k, got, exp)


# --------------------------------------------------------------------------
# ABI behaviour
# --------------------------------------------------------------------------
def raw_create(ops, sess, types, part, n_part, sort, sort_desc, n_sort, specs, n_specs,
               null_session=False, null_types=False, null_out=False):
    """tg_window_create with every pointer and count under the caller's control"""
    from trino_amd import _lib, _check
    ty = np.array(types, np.int32)
    arr = lambda v: None if v is None else np.array(v, np.int32)      # noqa: E731
    pc, sc, sd = arr(part), arr(sort), arr(sort_desc)
    sp = None
    if specs is not None:
        sp = (ops.TgWindowSpec * max(len(specs), 1))()
        for i, (fn, ch, fr) in enumerate(specs):
            sp[i].fn, sp[i].input_channel, sp[i].frame = fn, ch, fr
    h = ctypes.c_void_p()
    ptr = lambda a: None if a is None else a.ctypes.data              # noqa: E731
    st = _lib.tg_window_create(None if null_session else sess._h,
                               None if null_types else ty.ctypes.data, len(ty),
                               ptr(pc), n_part, ptr(sc), ptr(sd), n_sort, sp, n_specs,
                               None if null_out else ctypes.byref(h))
    assert (st == 0) == bool(h.value)
    if h.value:
        _lib.tg_operator_close(h)
    _check(st)


def test_rejections_by_status(sess, ops):
    B, D, V = ops.TG_BIGINT, ops.TG_DOUBLE, ops.TG_VARCHAR
    rn = [(ROW_NUMBER, -1, RANGE)]
    ok = dict(types=[B, B], part=[0], n_part=1, sort=[1], sort_desc=[0], n_sort=1, specs=rn,
              n_specs=1)
    raw_create(ops, sess, **ok)                                   # the base case is accepted
    inv = lambda **kw: expect_error(lambda: raw_create(ops, sess, **{**ok, **kw}),   # noqa: E731
                                    TG_ERR_INVALID_ARG)
    inv(null_session=True)
    inv(null_types=True)
    inv(null_out=True)
    inv(part=None)                      # null arrays with a non-zero count
    inv(sort=None)
    inv(sort_desc=None)
    inv(specs=None)
    inv(n_specs=0)
    inv(specs=rn * 9, n_specs=9)
    for ch in (-1, 2, 7):
        inv(part=[ch])
        inv(sort=[ch])
        inv(specs=[(SUM_I64, ch, ROWS)])
        inv(specs=[(COUNT_COL, ch, RANGE)])
    inv(specs=[(-1, 0, RANGE)])
    inv(specs=[(8, 0, RANGE)])
    inv(specs=[(SUM_I64, 0, -1)])
    inv(specs=[(SUM_I64, 0, 3)])
    for fn in (ROW_NUMBER, RANK, DENSE_RANK):
        for fr in (ROWS, PARTITION):
            inv(specs=[(fn, -1, fr)])
    uns = lambda word, **kw: expect_error(lambda: raw_create(ops, sess, **{**ok, **kw}),  # noqa: E731
                                          TG_ERR_UNSUPPORTED, word)
    uns("VARCHAR", types=[B, V], sort=[0])
    uns("VARCHAR", types=[V, B], part=[1])
    for fn in (SUM_I64, MIN_I64, MAX_I64, COUNT_COL):
        uns("DOUBLE", types=[B, D], specs=[(fn, 1, ROWS)])
    # a DOUBLE key or payload is fine, and so are zero counts with null arrays
    raw_create(ops, sess, **{**ok, "types": [D, D]})
    raw_create(ops, sess, **{**ok, "part": None, "n_part": 0, "sort": None, "sort_desc": None,
                             "n_sort": 0})
    # up to eight specs
    raw_create(ops, sess, **{**ok, "specs": rn * 8, "n_specs": 8})


def test_add_input_rejections_and_state_machine(sess, ops):
    B = ops.TG_BIGINT
    op = ops.window(sess, [B, B], [0], [1], [0], [(ROW_NUMBER, -1, RANGE)])
    try:
        narrow = [Col("i64", [1, 2]), Col("i32", [1, 2])]
        expect_error(lambda: op.add_input(make_page(ops, narrow)), TG_ERR_INVALID_ARG, "window")
        expect_error(lambda: op.add_input(make_page(ops, narrow[:1])), TG_ERR_INVALID_ARG,
                     "window")
        good = [Col("i64", [2, 1, 2]), Col("i64", [5, 6, 4])]
        op.add_input(make_page(ops, good))
        assert op.get_output() == (None, False)          # before finish: no page
        op.finish()
        expect_error(lambda: op.add_input(make_page(ops, good)), TG_ERR_STATE)
        cols, fin = op.get_output()
        assert not fin and cols[0]["values"].tolist() == [1, 2, 2]
        assert cols[1]["values"].tolist() == [6, 4, 5] and cols[2]["values"].tolist() == [1, 1, 2]
        assert op.get_output() == (None, True)
        assert op.get_output() == (None, True)
    finally:
        op.close()


def test_memory_returns_after_close(sess, ops):
    """live pool bytes (total - cached) after close equal the starting value:
    with output fetched, with output staged but not fetched, and closed
    without finish"""
    from trino_amd import session_memory

    def live():
        total, cached = session_memory(sess)
        return total - cached

    cols = layout_cols("p64", 2 * C + 1, 71)
    types = [tg_type(ops, c.kind) for c in cols]
    start = live()
    for mode in ("drained", "staged", "unfinished", "rejected_page"):
        op = ops.window(sess, types, [0], [1], [0], SPEC_GROUPS[1])
        op.add_input(make_page(ops, cols))
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
