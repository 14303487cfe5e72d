"""Window frame layer parity matrix (tg_window_create_ex in
trino_amd/csrc/ops_window.hip through trino_amd.ops.window_ex): bounded ROWS
frames and lag / lead / first_value / last_value / nth_value, bit-exact
against the references of tests/test_window_frames_reference.py:
ref_window_ex (plain Python) up to PLAIN_EX_ROWS rows, its numpy twin
ref_window_ex_vec above (the two are asserted equal there at every frame used
here).

As in tests/test_gpu_window_matrix.py every case carries a unique BIGINT
row-id payload channel (the last input channel) and asserts (1) the output
row order, (2) every payload cell and validity bit, (3) every spec column's
values, compared as int64 bits (a DOUBLE value column by its bits), and (4)
its validity, with a bitmap present exactly for SUM / MIN / MAX and the value
functions, and the output channel's type: the input channel's for a value
function, BIGINT otherwise. The layouts are those of the first matrix: they
put partition edges on the 64-row and WSCAN_CHUNK edges, so frames are cut on
one side, on both sides and inside a single chunk.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_filter_matrix import (Col, KINDS, _NP, POISON, expect_error, make_page, rows_of,
                                    tg_type, unpack_bits, TG_ERR_INVALID_ARG,
                                    TG_ERR_UNSUPPORTED)
from test_gpu_ordering_matrix import page_sizes, slice_cols, special_cols
from test_gpu_window_matrix import (C, DEEP_ROWS, EDGE_SIZES, LAYOUTS, SPEC_GROUPS,
                                    WAVE_CARRIES_ROWS, layout_cols, run_window)
from test_window_reference import (COUNT_COL, COUNT_STAR, I64_MAX, I64_MIN, MAX_I64,
                                   MIN_I64, PARTITION, RANGE, RANK, ROW_NUMBER, ROWS, SUM_I64,
                                   as_arrays, ref_window, table_cols)
from test_window_frames_reference import (FIRST_VALUE, FRAME_TABLES, FRAMES, LAG, LAST_VALUE,
                                          LEAD, NTH_VALUE, ROWS_BETWEEN, UNB_F, UNB_P,
                                          as_arrays_ex, assert_same_ex, ex, frame_specs,
                                          has_validity_ex, is_value_fn, ref_window_ex,
                                          ref_window_ex_vec, widen)

pytestmark = pytest.mark.gpu

RB = ROWS_BETWEEN
PLAIN_EX_ROWS = 65          # ref_window_ex up to here, ref_window_ex_vec above


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
def run_window_ex(sess, ops, cols, part, sort, desc, specs, sizes):
    op = ops.window_ex(sess, [tg_type(ops, c.kind) for c in cols], part, sort, desc, specs)
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


def spec_columns(ops, out, cols, specs):
    """the spec channels of an output page as (int64 bits, valid or None),
    after checking each channel's type and bitmap presence"""
    n = len(cols[0])
    got = []
    for k, sp in enumerate(specs):
        o = out[len(cols) + k]
        kind = cols[sp[1]].kind if is_value_fn(sp[0]) else "i64"
        assert o["type"] == tg_type(ops, kind), f"spec {k}: channel type {o['type']}"
        assert (o["valid"] is not None) == has_validity_ex(sp[0]), f"spec {k}: bitmap presence"
        vals = np.asarray(o["values"])
        assert vals.dtype.itemsize == np.dtype(_NP[kind]).itemsize, f"spec {k}: cell width"
        bits = vals.view(np.int64) if kind == "f64" else vals.astype(np.int64)
        got.append((bits, None if o["valid"] is None else unpack_bits(o["valid"], n)))
    return got


def check_window_ex(sess, ops, cols, part, sort, desc, specs, sizes=None, plain=None):
    """cols: the LAST column is the unique BIGINT row id"""
    n = len(cols[0])
    sizes = page_sizes(n) if sizes is None else sizes
    pages = run_window_ex(sess, ops, cols, part, sort, desc, specs, sizes)
    if n == 0:
        assert pages == []
        return None
    assert len(pages) == 1 and len(pages[0]) == len(cols) + len(specs)
    out = pages[0]
    if plain is None:
        plain = n <= PLAIN_EX_ROWS
    if plain:
        order, ref_cols = ref_window_ex(rows_of(cols), part, sort, desc, specs)
        exp = (np.array(order, np.int64), as_arrays_ex(ref_cols, specs, [c.kind for c in cols]))
    else:
        exp = ref_window_ex_vec(cols, part, sort, desc, specs)
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
    got = spec_columns(ops, out, cols, specs)
    assert_same_ex((rid, got), exp, specs, f"n={n}")
    return got


def groups_of_eight(specs):
    return [specs[i:i + 8] for i in range(0, len(specs), 8)]


# --------------------------------------------------------------------------
# frames x layouts
# --------------------------------------------------------------------------
def test_frame_list_reaches_every_path():
    """lengths 2^k - 1, 2^k and 2^k + 1 at the wave and the chunk, frames open
    at one end and at both, an always-empty frame, saturating offsets"""
    assert len(FRAMES) == 22 and len(set(FRAMES)) == 22
    widths = {e - s + 1 for s, e in FRAMES if UNB_P < s <= e < UNB_F}
    assert {1, 2, 3, 4, 7, 63 + 1, 64 + 1, 1024, 1025, 1401} <= widths
    assert (3, 1) in FRAMES and (UNB_P, UNB_F) in FRAMES
    assert any(s == UNB_P and e < 0 for s, e in FRAMES) and any(s > 0 and e == UNB_F for s, e in FRAMES)
    assert len(frame_specs(0, 0)) == 8       # the ABI's limit: one operator per frame


@pytest.mark.parametrize("n", EDGE_SIZES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_layouts_every_aggregate_and_frame(sess, ops, name, n):
    """every aggregate on the nullable BIGINT channel and first / last /
    nth_value on the nullable DOUBLE channel, under each ROWS BETWEEN frame"""
    cols = layout_cols(name, n, 2000 + n)
    for start, end in FRAMES:
        check_window_ex(sess, ops, cols, [0], [1], [0], frame_specs(start, end, x=2, v=4))


@pytest.mark.parametrize("name", ["long", "p64", "late_nonnull"])
def test_layouts_small_input_and_no_partition_channel(sess, ops, name):
    """the SMALLINT channel as aggregate and value input; then the same rows
    as one partition of everything, sorted descending"""
    cols = layout_cols(name, 2 * C + 1, 17)
    for start, end in ((-6, 0), (-64, 0), (-700, 700), (-3, UNB_F), (UNB_P, 3)):
        check_window_ex(sess, ops, cols, [0], [1], [0], frame_specs(start, end, x=3, v=3))
        check_window_ex(sess, ops, cols, [], [1, 0], [1, 0], frame_specs(start, end, x=2, v=1))


# --------------------------------------------------------------------------
# old specs through the new entry
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_old_specs_through_the_new_entry(sess, ops, n):
    """ALL_SPECS through window_ex: equal to ref_window, and the same bits as
    through ops.window"""
    for name in ("long", "edges", "last_alone"):
        cols = layout_cols(name, n, 3000 + n)
        rows = rows_of(cols)
        for specs in SPEC_GROUPS:
            pages = run_window_ex(sess, ops, cols, [0], [1], [0], widen(specs), page_sizes(n))
            assert len(pages) == 1
            got = spec_columns(ops, pages[0], cols, widen(specs))
            rid = np.asarray(pages[0][len(cols) - 1]["values"], np.int64)
            order, ref_cols = ref_window(rows, [0], [1], [0], specs)
            assert_same_ex((rid, got), (np.array(order, np.int64), as_arrays(ref_cols, specs)),
                           widen(specs), f"{name} n={n}")
            old = run_window(sess, ops, cols, [0], [1], [0], specs, page_sizes(n))[0]
            for a, b in zip(pages[0], old):
                assert a["type"] == b["type"] and (a["valid"] is None) == (b["valid"] is None)
                assert np.array_equal(np.asarray(a["values"]).view(np.uint8),
                                      np.asarray(b["values"]).view(np.uint8))
                assert a["valid"] is None or np.array_equal(a["valid"], b["valid"])


def test_old_and_new_specs_in_one_operator(sess, ops):
    """the shared intermediates (row_number, frame ends, the input's count)
    serve both kinds of spec"""
    cols = layout_cols("long", 2 * C + 1, 19)
    specs = [ex(SUM_I64, 2, RANGE), ex(SUM_I64, 2, RB, -6, 0), ex(MIN_I64, 2, ROWS),
             ex(MIN_I64, 2, RB, -6, 0), ex(LEAD, 2, offset=1), ex(COUNT_STAR, -1, PARTITION),
             ex(LAST_VALUE, 2, RANGE), ex(RANK)]
    check_window_ex(sess, ops, cols, [0], [1], [0], specs)


# --------------------------------------------------------------------------
# lag / lead
# --------------------------------------------------------------------------
def lag_lead_specs(ch, n):
    ks = (0, 1, 2, 63, 64, 65, 1024, 1025, max(n - 1, 0), n, 2 ** 62)
    return [ex(fn, ch, offset=k) for fn in (LAG, LEAD) for k in ks]


@pytest.mark.parametrize("n", EDGE_SIZES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_lag_lead_by_layout(sess, ops, name, n):
    """a DOUBLE input with NaN payloads, -0.0 and NULLs, compared as bits"""
    cols = layout_cols(name, n, 4000 + n)
    cols[4] = special_cols("double_specials", n, 4100 + n)
    for specs in groups_of_eight(lag_lead_specs(4, n)):
        check_window_ex(sess, ops, cols, [0], [1], [0], specs)


def typed_input(kind, n, seed):
    r = np.random.default_rng(seed)
    if kind == "f64":
        return special_cols("double_specials", n, seed)
    if kind == "bool":
        vals = r.integers(0, 2, n)
    else:
        info = np.iinfo(_NP[kind])
        vals = r.integers(info.min, info.max, n, endpoint=True)
        vals[:2] = (info.min, info.max)
    null = r.random(n) < 0.3
    vals = np.asarray(vals, _NP[kind])
    vals[null] = POISON[kind]
    return Col(kind, vals, ~null)


@pytest.mark.parametrize("kind", KINDS)
def test_every_type_as_value_input(sess, ops, kind):
    """every fixed-width type through every value function; the output
    channel keeps the input's type and width (spec_columns asserts both)"""
    n = C + 1
    r = np.random.default_rng(5)
    cols = [Col("i32", np.sort(r.integers(0, 9, n))), typed_input(kind, n, 6),
            Col("i64", np.arange(n))]
    specs = [ex(LAG, 1, offset=1), ex(LEAD, 1, offset=65), ex(FIRST_VALUE, 1, RB, -6, 0),
             ex(LAST_VALUE, 1, RB, -3, 70), ex(NTH_VALUE, 1, RB, -64, 64, 64),
             ex(FIRST_VALUE, 1, RANGE), ex(LAST_VALUE, 1, PARTITION), ex(NTH_VALUE, 1, ROWS, offset=2)]
    check_window_ex(sess, ops, cols, [0], [2], [1], specs)


# --------------------------------------------------------------------------
# nth_value
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, C + 1, 2 * C + 1])
@pytest.mark.parametrize("name", ["one", "p64", "long", "edges"])
def test_nth_value_under_every_frame_kind(sess, ops, name, n):
    cols = layout_cols(name, n, 5000 + n)
    specs = [ex(NTH_VALUE, 4, fr, s, e, k)
             for fr, s, e in ((RANGE, 0, 0), (ROWS, 0, 0), (PARTITION, 0, 0), (RB, -1024, 1024))
             for k in (1, 2, 64, 65, 1025, 2 ** 62)]
    for group in groups_of_eight(specs):
        check_window_ex(sess, ops, cols, [0], [1], [0], group)


# --------------------------------------------------------------------------
# NULLs
# --------------------------------------------------------------------------
NULL_FRAMES = ((-6, 0), (-700, 700), (UNB_P, 0), (-3, UNB_F), (0, 0))


def test_all_null_input(sess, ops):
    """every sum / min / max NULL and every count 0, under the level kernel,
    both one-sided forms and the prefix difference"""
    n = 2 * C + 1
    cols = layout_cols("long", n, 23)
    cols[2] = Col("i64", np.full(n, POISON["i64"]), np.zeros(n, bool))
    for start, end in NULL_FRAMES:
        specs = [ex(fn, 2, RB, start, end) for fn in (SUM_I64, MIN_I64, MAX_I64, COUNT_COL)]
        got = check_window_ex(sess, ops, cols, [0], [1], [0], specs)
        for vals, valid in got[:3]:
            assert not valid.any()
        assert not got[3][0].any() and got[3][1] is None


def test_frames_without_a_non_null_cell(sess, ops):
    """one non-NULL cell in 50: most narrow frames hold none and are NULL,
    the frames around a non-NULL cell are not"""
    n = 2 * C + 1
    cols = layout_cols("long", n, 24)
    present = cols[2].valid & (np.arange(n) % 50 == 0)
    cols[2] = Col("i64", np.where(present, cols[2].values, POISON["i64"]), present)
    for start, end in NULL_FRAMES:
        specs = [ex(fn, 2, RB, start, end) for fn in (SUM_I64, MIN_I64, MAX_I64, COUNT_COL)]
        got = check_window_ex(sess, ops, cols, [0], [1], [0], specs)
        if (start, end) == (-6, 0):
            assert got[1][1].any() and not got[1][1].all()


def test_null_at_the_frame_edge_is_a_null_value(sess, ops):
    """first_value / last_value return the NULL at lo / hi; they do not skip
    to the next non-NULL cell"""
    n = C + 1
    present = np.arange(n) % 2 == 1                       # sorted positions 0, 2, 4 .. are NULL
    cols = [Col("i64", np.zeros(n, np.int64)), Col("i64", np.arange(n) * 10, present),
            Col("i64", np.arange(n))]
    specs = [ex(FIRST_VALUE, 1, RB, -1, 0), ex(LAST_VALUE, 1, RB, 0, 1), ex(FIRST_VALUE, 1, ROWS),
             ex(LAST_VALUE, 1, PARTITION), ex(NTH_VALUE, 1, RB, -2, 0, 2)]
    got = check_window_ex(sess, ops, cols, [0], [2], [0], specs)
    pos = np.arange(n)
    assert np.array_equal(got[0][1], (pos % 2 == 0) & (pos > 0))      # the cell at i - 1
    assert np.array_equal(got[1][1], (pos % 2 == 0) & (pos < n - 1))  # the cell at i + 1
    assert not got[2][1].any()                                        # the cell at 0 is NULL
    assert not present[n - 1] and not got[3][1].any()                 # the cell at n - 1 is NULL


def test_min_max_identity_next_to_nulls(sess, ops):
    """real INT64_MAX / INT64_MIN cells among NULLs: the identity that stands
    in for a NULL must not decide validity"""
    n = 2 * C + 1
    r = np.random.default_rng(25)
    pool = np.array([I64_MAX, I64_MIN, I64_MAX, I64_MIN, 0, -1], np.int64)
    x = pool[r.integers(0, len(pool), n)]
    null = r.random(n) < 0.6
    x[null] = POISON["i64"]
    cols = [Col("i64", r.integers(0, 5, n)), Col("i64", x, ~null), Col("i64", np.arange(n))]
    for start, end in ((0, 0), (-1, 0), (-6, 0), (-64, 64), (UNB_P, 1), (-2, UNB_F)):
        specs = [ex(fn, 1, RB, start, end) for fn in (MIN_I64, MAX_I64, SUM_I64, COUNT_COL)]
        check_window_ex(sess, ops, cols, [0], [2], [0], specs)
        check_window_ex(sess, ops, cols, [0], [2], [0], specs, plain=True)


@pytest.mark.parametrize("name", sorted(FRAME_TABLES))
def test_hand_written_tables(sess, ops, name):
    """the typed-out expectations of test_window_frames_reference, on the device"""
    t = FRAME_TABLES[name]
    cols = table_cols(t["rows"])
    n = len(t["rows"])
    cols.append(Col("i64", np.arange(n)))
    pages = run_window_ex(sess, ops, cols, t["part"], t["sort"], t["desc"], t["specs"], (n,))
    out = pages[0]
    assert out[len(cols) - 1]["values"].tolist() == t["order"]
    got = spec_columns(ops, out, cols, t["specs"])
    exp = as_arrays_ex(t["cols"], t["specs"], [c.kind for c in cols])
    assert_same_ex((t["order"], got), (t["order"], exp), t["specs"], name)


# --------------------------------------------------------------------------
# depth
# --------------------------------------------------------------------------
DEEP_SPECS = [ex(SUM_I64, 2, RB, -6, 0), ex(MIN_I64, 2, RB, -6, 0), ex(SUM_I64, 2, RB, -700, 700),
              ex(MIN_I64, 2, RB, -700, 700), ex(LAG, 2, offset=1)]


def deep_cols(n, partitions, seed):
    """[partition key, sort key, x nullable, row id]; partitions of equal
    length, so with 2^10 of them at DEEP_ROWS no edge sits on a chunk edge"""
    r = np.random.default_rng(seed)
    pos = np.arange(n, dtype=np.int64)
    present = r.random(n) >= 0.3
    x = r.integers(-10 ** 12, 10 ** 12, n)
    x[~present] = POISON["i64"]
    shuffle = r.permutation(n)
    cols = [Col("i64", pos * partitions // n), Col("i64", pos), Col("i64", x, present)]
    cols = [Col(c.kind, c.values[shuffle], None if c.valid is None else c.valid[shuffle])
            for c in cols]
    return cols + [Col("i64", np.arange(n))]


@pytest.mark.parametrize("partitions", [1, 1 << 10])
def test_deep_rows(sess, ops, partitions):
    """2^20 + 1 rows, where the carry scan behind the prefix sums recurses and
    the level kernel's grid-stride loop makes more than one trip"""
    cols = deep_cols(DEEP_ROWS, partitions, 31)
    check_window_ex(sess, ops, cols, [0], [1], [0], DEEP_SPECS)


def test_one_more_carry_than_a_wave(sess, ops):
    cols = deep_cols(WAVE_CARRIES_ROWS, 37, 32)
    check_window_ex(sess, ops, cols, [0], [1], [0],
                    DEEP_SPECS + [ex(MAX_I64, 2, RB, -1024, 0), ex(LEAD, 2, offset=1025),
                                  ex(LAST_VALUE, 2, RB, 2, 5)])


# --------------------------------------------------------------------------
# pages
# --------------------------------------------------------------------------
def test_multi_page_input(sess, ops):
    specs = frame_specs(-6, 0, x=2, v=4)[:6] + [ex(LAG, 4, offset=1), ex(LEAD, 2, offset=2)]
    cols = layout_cols("pairs", 65, 41)
    check_window_ex(sess, ops, cols, [0], [1], [0], specs, sizes=(0, 64, 0, 1, 0))
    cols = layout_cols("long", 2 * C + 1, 42)
    for sizes in ((2 * C + 1,), page_sizes(2 * C + 1), (C, 0, 1, C), (63, 64, 65, 2 * C + 1 - 192)):
        check_window_ex(sess, ops, cols, [0], [1], [0], specs, sizes=sizes)


def test_empty_input(sess, ops):
    cols = [c for c in layout_cols("one", 0, 43)]
    for sizes in ((), (0,), (0, 0)):
        assert check_window_ex(sess, ops, cols, [0], [1], [0], frame_specs(-6, 0, x=2, v=4),
                               sizes=sizes) is None


# --------------------------------------------------------------------------
# ABI behaviour
# --------------------------------------------------------------------------
def raw_create_ex(ops, sess, types, part, n_part, sort, sort_desc, n_sort, specs, n_specs,
                  null_session=False, null_types=False, null_out=False):
    """tg_window_create_ex with every pointer and count under the caller's control"""
    from trino_amd import _lib, _check
    ty = np.array(types, np.int32)
    arr = lambda v: None if v is None else np.array(v, np.int32)      # noqa: E731
    pc, sc, sd = arr(part), arr(sort), arr(sort_desc)
    sp = None
    if specs is not None:
        sp = (ops.TgWindowSpecEx * max(len(specs), 1))()
        for i, (fn, ch, fr, start, end, offset) in enumerate(specs):
            sp[i].fn, sp[i].input_channel, sp[i].frame = fn, ch, fr
            sp[i].frame_start, sp[i].frame_end, sp[i].offset = start, end, offset
    h = ctypes.c_void_p()
    ptr = lambda a: None if a is None else a.ctypes.data              # noqa: E731
    st = _lib.tg_window_create_ex(None if null_session else sess._h,
                                  None if null_types else ty.ctypes.data, len(ty),
                                  ptr(pc), n_part, ptr(sc), ptr(sd), n_sort, sp, n_specs,
                                  None if null_out else ctypes.byref(h))
    assert (st == 0) == bool(h.value)
    if h.value:
        _lib.tg_operator_close(h)
    _check(st)


def test_rejections_by_status(sess, ops):
    B, D, V = ops.TG_BIGINT, ops.TG_DOUBLE, ops.TG_VARCHAR
    rn = [ex(ROW_NUMBER)]
    ok = dict(types=[B, B], part=[0], n_part=1, sort=[1], sort_desc=[0], n_sort=1, specs=rn,
              n_specs=1)
    raw_create_ex(ops, sess, **ok)                                # the base case is accepted
    inv = lambda **kw: expect_error(lambda: raw_create_ex(ops, sess, **{**ok, **kw}),   # noqa: E731
                                    TG_ERR_INVALID_ARG)
    one = lambda *a, **kw: inv(specs=[ex(*a, **kw)])              # noqa: E731
    # what tg_window_create rejects
    inv(null_session=True)
    inv(null_types=True)
    inv(null_out=True)
    inv(part=None)
    inv(sort=None)
    inv(sort_desc=None)
    inv(specs=None)
    inv(n_specs=0)
    inv(specs=rn * 9, n_specs=9)
    for ch in (-1, 2, 7):
        inv(part=[ch])
        inv(sort=[ch])
        one(SUM_I64, ch, ROWS)
        one(COUNT_COL, ch, RANGE)
        for fn in (LAG, LEAD, FIRST_VALUE, LAST_VALUE, NTH_VALUE):    # a value function's input
            one(fn, ch, RANGE, offset=0 if fn in (FIRST_VALUE, LAST_VALUE) else 1)
    one(-1, 0)
    one(13, 0)                          # fn outside 0..12
    one(SUM_I64, 0, -1)
    one(SUM_I64, 0, 4)                  # frame outside 0..3
    for fn in (ROW_NUMBER, RANK):
        for fr in (ROWS, PARTITION, RB):
            one(fn, -1, fr)
    for fn in (LAG, LEAD):              # lag / lead take frame 0
        for fr in (ROWS, PARTITION, RB):
            one(fn, 0, fr, offset=1)
        one(fn, 0, offset=-1)           # offset < 0
        one(fn, 0, offset=I64_MIN)
    for k in (0, -1, I64_MIN):          # nth_value counts from 1
        one(NTH_VALUE, 0, ROWS, offset=k)
    for fn in (ROW_NUMBER, COUNT_STAR, SUM_I64, FIRST_VALUE, LAST_VALUE):
        one(fn, 0, RANGE, offset=1)     # an offset on a function that takes none
        one(fn, 0, RANGE, offset=-1)
    one(SUM_I64, 0, RB, UNB_F, UNB_F)   # a frame cannot start at UNBOUNDED FOLLOWING
    one(SUM_I64, 0, RB, UNB_P, UNB_P)   # nor end at UNBOUNDED PRECEDING
    one(FIRST_VALUE, 0, RB, UNB_F, 0)
    one(FIRST_VALUE, 0, RB, 0, UNB_P)
    for fr in (RANGE, ROWS, PARTITION): # frame offsets belong to ROWS_BETWEEN
        one(SUM_I64, 0, fr, -1, 0)
        one(SUM_I64, 0, fr, 0, 1)
        one(LAST_VALUE, 0, fr, UNB_P, 0)
    uns = lambda word, **kw: expect_error(lambda: raw_create_ex(ops, sess, **{**ok, **kw}),  # noqa: E731
                                          TG_ERR_UNSUPPORTED, word)
    uns("VARCHAR", types=[B, V], sort=[0])
    uns("VARCHAR", types=[V, B], part=[1])
    uns("VARCHAR", types=[B, V], sort=[0], specs=[ex(LAG, 1, offset=1)])
    for fn in (SUM_I64, MIN_I64, MAX_I64, COUNT_COL):
        uns("DOUBLE", types=[B, D], specs=[ex(fn, 1, RB, -1, 0)])
        uns("DOUBLE", types=[B, D], specs=[ex(fn, 1, ROWS)])
    # accepted: a DOUBLE value input, an always-empty frame, saturating offsets, eight specs
    fine = lambda specs, **kw: raw_create_ex(ops, sess, **{**ok, "specs": specs,   # noqa: E731
                                                        "n_specs": len(specs), **kw})
    fine([ex(fn, 1, RANGE, offset=1) for fn in (LAG, LEAD, NTH_VALUE)], types=[B, D])
    fine([ex(SUM_I64, 0, RB, 3, 1), ex(MIN_I64, 0, RB, 2 ** 62, I64_MAX - 1),
          ex(MAX_I64, 0, RB, I64_MIN + 1, -2 ** 62), ex(COUNT_STAR, -1, RB, UNB_P, UNB_F)])
    fine([ex(LAG, 0, offset=0), ex(LEAD, 0, offset=I64_MAX), ex(NTH_VALUE, 0, RB, -1, 1, I64_MAX)])
    fine(rn * 8)
    raw_create_ex(ops, sess, **{**ok, "part": None, "n_part": 0, "sort": None, "sort_desc": None,
                                "n_sort": 0})


def test_memory_returns_after_close(sess, ops):
    """live pool bytes after close equal the starting value: drained, staged,
    unfinished, and after a rejected page"""
    from trino_amd import session_memory

    def live():
        total, cached = session_memory(sess)
        return total - cached

    cols = layout_cols("p64", 2 * C + 1, 71)
    types = [tg_type(ops, c.kind) for c in cols]
    specs = [ex(SUM_I64, 2, RB, -6, 0), ex(MIN_I64, 2, RB, -700, 700), ex(MAX_I64, 2, RB, -3, UNB_F),
             ex(LAG, 4, offset=1), ex(LEAD, 3, offset=2), ex(NTH_VALUE, 4, RB, -6, 0, 2),
             ex(SUM_I64, 2, RANGE), ex(RANK)]
    start = live()
    for mode in ("drained", "staged", "unfinished", "rejected_page"):
        op = ops.window_ex(sess, types, [0], [1], [0], specs)
        op.add_input(make_page(ops, cols))
        assert live() > start
        if mode == "drained":
            assert len(op.drain()) == 1
        elif mode == "staged":
            op.finish()
            assert op.get_output()[0] is not None
        elif mode == "rejected_page":
            expect_error(lambda: op.add_input(make_page(ops, cols[:2])), TG_ERR_INVALID_ARG)
        op.close()
        assert live() == start, mode
