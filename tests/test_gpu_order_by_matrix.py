"""Parity matrix of the OrderBy operator and of TopN with VARCHAR channels
(tg_order_by_create / tg_topn_create_ex, trino_amd/csrc/ops_topn.hip) against
the exact plain-Python reference ref_order_by of test_order_by_reference.

What runs underneath: order_pages with the rank image of a VARCHAR key
(k_var_lens, k_var_chunks, k_var_flags, k_var_scatter_ranks, k_var_finish and
the length round; sort.hip) and gather_pages with a VARCHAR
channel over several source pages (k_pages_var_lens, run_scan_i32,
k_pages_var_copy at each lane count).

Every case carries a unique BIGINT row id as its last channel and is checked
bit for bit: the row order (whole-key ties in input order), every payload
cell, every validity bit and whether the bitmap exists at all, and for
VARCHAR outputs offsets[0] == 0 and diff(offsets) == the expected lengths.
NULL cells carry poison values that would sort or read wrongly if used.
"""
import ctypes
import math

import numpy as np
import pytest

from test_gpu_filter_matrix import (Col, _NP, expect_error, make_page, rows_of, tg_type,
                                    unpack_bits, TG_ERR_INVALID_ARG, TG_ERR_UNSUPPORTED)
from test_gpu_ordering_matrix import page_sizes, slice_cols, wide_pages
from test_order_by_reference import ADVERSARIAL, ref_order_by

pytestmark = pytest.mark.gpu

FSCAN_CHUNK = 2048          # ops_filter.hip; pinned by the filter matrix
POISON_STR = b"\x00<poison>\xff"


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
# runner and checker
# --------------------------------------------------------------------------
def split(cols, sizes):
    pages, at = [], 0
    for n in sizes:
        pages.append(slice_cols(cols, at, at + n))
        at += n
    assert at == len(cols[0])
    return pages


def run_pages(op, ops, pages):
    try:
        for cols in pages:
            op.add_input(make_page(ops, cols))
        return op.drain()
    finally:
        op.close()


def check_pages(sess, ops, pages, sort, desc, limit=None, out_channels=None):
    """pages: lists of Col, the same kinds in every page; the last channel is
    the unique BIGINT row id. Returns the output row ids."""
    types = [tg_type(ops, c.kind) for c in pages[0]]
    if limit is None:
        op = ops.order_by(sess, types, sort, desc, out_channels)
    else:
        assert out_channels is None
        op = ops.topn_ex(sess, types, sort, desc, limit)
    got_pages = run_pages(op, ops, pages)
    rows = [r for cols in pages for r in rows_of(cols)]
    n = len(rows)
    if n == 0:
        assert got_pages == []
        return []
    order = np.array(ref_order_by(rows, sort, desc, limit), np.int64)
    take = len(order)
    assert take == (n if limit is None else min(limit, n))
    channels = list(range(len(types))) if out_channels is None else list(out_channels)
    assert len(got_pages) == 1 and len(got_pages[0]) == len(channels)
    out = got_pages[0]
    for k, c in enumerate(channels):
        kind = pages[0][c].kind
        what = f"output {k} (channel {c}, {kind})"
        assert out[k]["type"] == types[c], what
        has_bitmap = any(len(p[c]) and p[c].valid is not None for p in pages)
        assert (out[k]["valid"] is not None) == has_bitmap, f"{what}: bitmap presence"
        svalid = np.concatenate([np.ones(len(p[c]), bool) if p[c].valid is None else p[c].valid
                                 for p in pages])
        gvalid = unpack_bits(out[k]["valid"], take)
        assert np.array_equal(gvalid, svalid[order]), f"{what}: validity"
        if kind == "str":
            flat = [v for p in pages for v in p[c].values]
            exp = [flat[i] if svalid[i] else b"" for i in order]
            assert len(out[k]["values"]) == take, what
            offs = out[k]["offsets"].astype(np.int64)
            assert offs[0] == 0, what
            assert np.array_equal(np.diff(offs), [len(x) for x in exp]), f"{what}: lengths"
            if out[k]["values"] != exp:
                j = next(i for i, (a, b) in enumerate(zip(out[k]["values"], exp)) if a != b)
                raise AssertionError(f"{what}: output row {j} is {out[k]['values'][j]!r}, "
                                     f"expected {exp[j]!r} (input row {order[j]})")
            continue
        view = np.int64 if kind == "f64" else _NP[kind]
        src = np.concatenate([p[c].values for p in pages])
        g = np.asarray(out[k]["values"])
        assert len(g) == take, what
        bad = np.flatnonzero((g.view(view) != src[order].view(view)) & gvalid)
        assert len(bad) == 0, (f"{what}: output row {bad[0]} holds {g[bad[0]]}, expected input "
                               f"row {order[bad[0]]}")
    rid_at = channels.index(len(types) - 1)
    return np.asarray(out[rid_at]["values"]).tolist()


def check(sess, ops, cols, sort, desc, sizes=None, **kw):
    n = len(cols[0])
    return check_pages(sess, ops, split(cols, page_sizes(n) if sizes is None else sizes),
                       sort, desc, **kw)


def with_rid(*cols):
    return list(cols) + [Col("i64", np.arange(len(cols[0])))]


def shuffled(values, seed):
    r = np.random.default_rng(seed)
    return [values[i] for i in r.permutation(len(values))]


def three_page_splits(n):
    """one page, then three pages with a zero-row page first, in the middle
    and last"""
    a = n // 3
    return [(n,), (0, a, n - a), (a, 0, n - a), (a, n - a, 0)]


# --------------------------------------------------------------------------
# adversarial strings as the only key
# --------------------------------------------------------------------------
def _last_byte_family():
    out = []
    for length in (7, 8, 9, 15, 16, 17):
        stem = b"q" * (length - 1)
        out += [stem + b"a", stem + b"b", stem + b"\0", stem + b"\xff", stem]
    return out


def _deep_prefix_family():
    """a 64-byte common prefix; strings differ at byte 64, 71 or 72: nine to
    ten chunk rounds"""
    p = b"z" * 64
    out = [p]
    for mid in (b"", b"m" * 7, b"m" * 8):
        out += [p + mid + x for x in (b"a", b"b", b"\0", b"\xff", b"a\0")]
    return out


STRING_SETS = {
    "documented": ADVERSARIAL * 3,
    "last_byte": _last_byte_family() * 2,
    "deep_prefix": _deep_prefix_family() * 2,
    "all_equal": [b"same string"] * 70,
    "all_distinct": [b"%05d" % i for i in range(300)],
    "trailing_zeros": [b"a" * 8 + bytes(k) for k in range(12)] + [bytes(k) for k in range(20)],
}


@pytest.mark.parametrize("desc", [0, 1])
@pytest.mark.parametrize("name", sorted(STRING_SETS))
def test_adversarial_string_key(sess, ops, name, desc):
    strs = shuffled(STRING_SETS[name], len(name))
    cols = with_rid(Col("str", strs))
    for sizes in three_page_splits(len(strs)):
        rid = check(sess, ops, cols, [0], [desc], sizes=sizes)
    if name == "all_equal":
        assert rid == list(range(len(strs)))              # ties keep input order
    if name == "documented" and not desc:
        assert [strs[i] for i in rid[::3]] == ADVERSARIAL


# --------------------------------------------------------------------------
# NULLs
# --------------------------------------------------------------------------
@pytest.mark.parametrize("desc", [0, 1])
def test_null_keys_separate_from_empty_strings(sess, ops, desc):
    r = np.random.default_rng(5 + desc)
    n = 200
    null = r.random(n) < 0.3
    pool = [b"", b"", b"\0", b"a"]
    strs = [POISON_STR if z else pool[k] for z, k in zip(null, r.integers(0, 4, n))]
    cols = with_rid(Col("str", strs, ~null))
    for sizes in three_page_splits(n):
        rid = check(sess, ops, cols, [0], [desc], sizes=sizes)
    nulls = int(null.sum())
    block = rid[:nulls] if desc else rid[n - nulls:]
    assert block == np.flatnonzero(null).tolist()          # NULLs together, in input order
    # only NULLs and no '' in the channel, and only NULLs at all
    cols = with_rid(Col("str", [POISON_STR, b"b", POISON_STR, b"a"], [0, 1, 0, 1]))
    assert check(sess, ops, cols, [0], [desc], sizes=(4,)) == ([0, 2, 1, 3] if desc else [3, 1, 0, 2])
    cols = with_rid(Col("str", [POISON_STR] * 5, [0] * 5))
    assert check(sess, ops, cols, [0], [desc]) == [0, 1, 2, 3, 4]


def test_bitmap_in_one_page_and_not_in_another(sess, ops):
    a = with_rid(Col("str", [b"b", POISON_STR, b""], [1, 0, 1]), Col("str", [b"x", b"y", b"z"]),
                 Col("i32", [1, 2, 3]))
    b = with_rid(Col("str", [b"a", b"", b"c"]), Col("str", [b"p", POISON_STR, b""], [1, 0, 1]),
                 Col("i32", [7, 7, 7], [1, 1, 0]))
    b[-1] = Col("i64", [3, 4, 5])
    empty_with_bitmap = with_rid(Col("str", [], []), Col("str", [], []), Col("i32", [], []))
    for desc in (0, 1):
        check_pages(sess, ops, [a, b], [0], [desc])
        check_pages(sess, ops, [b, a], [0, 1], [desc, 1 - desc])
    # a zero-row page's bitmap does not count: no channel of the output has one
    plain = with_rid(Col("str", [b"b", b"a"]), Col("str", [b"", b"q"]), Col("i32", [1, 2]))
    check_pages(sess, ops, [empty_with_bitmap, plain], [0], [0])


# --------------------------------------------------------------------------
# several keys
# --------------------------------------------------------------------------
def multi_cols(n, seed):
    r = np.random.default_rng(seed)
    words = [b"", b"a", b"a\0", b"ab", b"brand#1", b"brand#12", b"\x80", b"m" * 20, b"m" * 20 + b"z"]
    null = r.random(n) < 0.1
    s1 = Col("str", [POISON_STR if z else words[k] for z, k in zip(null, r.integers(0, 9, n))],
             ~null)
    null2 = r.random(n) < 0.1
    s2 = Col("str", [b"zzzz" if z else words[k] for z, k in zip(null2, r.integers(0, 4, n))],
             ~null2)
    i = Col("i64", r.integers(-3, 4, n), r.random(n) >= 0.1)
    fpool = np.array([0.0, -0.0, math.nan, -math.nan, 1.5, -math.inf, math.inf])
    f = Col("f64", fpool[r.integers(0, 7, n)], r.random(n) >= 0.1)
    return with_rid(s1, s2, i, f)


MULTI = {"varchar_bigint_desc": ([0, 2], [0, 1]),
         "bigint_desc_varchar_double": ([2, 0, 3], [1, 0, 0]),
         "bigint_varchar_desc_double_desc": ([2, 1, 3], [0, 1, 1]),
         "two_varchars_opposite": ([0, 1], [0, 1]),
         "two_varchars_opposite_swapped": ([1, 0], [0, 1])}


@pytest.mark.parametrize("name", sorted(MULTI))
def test_multi_key(sess, ops, name):
    sort, desc = MULTI[name]
    cols = multi_cols(700, len(name))
    check(sess, ops, cols, sort, desc)
    check(sess, ops, cols, sort, desc, sizes=(700,))


# --------------------------------------------------------------------------
# row counts
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1025, 2 * FSCAN_CHUNK + 1])
def test_row_counts(sess, ops, n):
    """a VARCHAR key with ties and NULLs and a VARCHAR payload; the last count
    takes the multi-block run_scan_i32 in the gather and in the refinement"""
    r = np.random.default_rng(n)
    pool = [b"k%03d" % i + b"\0" * (i % 3) for i in range(37)]
    null = r.random(n) < 0.1
    key = Col("str", [POISON_STR if z else pool[k] for z, k in zip(null, r.integers(0, 37, n))],
              ~null)
    pay = Col("str", [b"%d" % i * (i % 5) for i in range(n)])
    for desc in (0, 1):
        check(sess, ops, with_rid(key, pay), [0], [desc])


def test_two_hundred_thousand_rows(sess, ops):
    """crosses the grid stride (2048 blocks of 256), 2^12 distinct 12-byte
    strings: two chunk rounds and a rank sort of 12 bits"""
    n = 200_000
    r = np.random.default_rng(12)
    distinct = r.permutation(np.unique(r.integers(0, 10 ** 7, 6000)))[:4096]
    pool = [b"cust#" + b"%07d" % v for v in distinct]
    assert len(set(pool)) == 4096
    key = Col("str", [pool[k] for k in r.integers(0, 4096, n)])
    rid = check(sess, ops, with_rid(key), [0], [0], sizes=(70_000, 0, 130_000))
    assert len(rid) == n


# --------------------------------------------------------------------------
# pages
# --------------------------------------------------------------------------
def test_only_zero_row_pages_give_no_output(sess, ops):
    empty = with_rid(Col("str", []), Col("f64", []))
    for pages in ([empty], [empty, empty, empty], []):
        types = [ops.TG_VARCHAR, ops.TG_DOUBLE, ops.TG_BIGINT]
        for op in (ops.order_by(sess, types, [0], [0]), ops.topn_ex(sess, types, [0], [1], 3)):
            assert run_pages(op, ops, pages) == []


# --------------------------------------------------------------------------
# payloads and output_channels
# --------------------------------------------------------------------------
def wide_with_rid(sizes, seed):
    pages, at = [], 0
    for cols in wide_pages(sizes, seed):
        n = len(cols[0])
        pages.append(cols + [Col("i64", np.arange(at, at + n))])
        at += n
    return pages


@pytest.mark.parametrize("sizes", [(900,), (400, 0, 500), (0, 1, 899)])
def test_every_payload_width_and_two_varchar_payloads(sess, ops, sizes):
    """wide_pages: INTEGER and DOUBLE keys, a payload of every fixed width
    with NULLs, a VARCHAR payload with NULLs over poison, '' and 70-byte
    strings, a VARCHAR payload of distinct strings"""
    pages = wide_with_rid(sizes, 21)
    check_pages(sess, ops, pages, [9, 0], [0, 1])       # the nullable VARCHAR, then INTEGER desc
    check_pages(sess, ops, pages, [0, 1], [1, 0])       # fixed-width keys, VARCHAR payloads only


@pytest.mark.parametrize("out_channels", [[11], [11, 10], [10, 2, 11, 10, 9, 9], [5, 11, 0]])
def test_output_channels(sess, ops, out_channels):
    """a subset, a reordering and a repeated channel; the sort channels (9, 1)
    are not always emitted"""
    pages = wide_with_rid((300, 0, 333), 4)
    check_pages(sess, ops, pages, [9, 1], [1, 0], out_channels=out_channels)


def test_long_strings_take_every_copy_width(sess, ops):
    """mean payload lengths of 3, 30, 100 and 400 bytes: k_pages_var_copy at
    the 4, 8, 16 and 32 lanes per row its table picks, and at every lane count
    it is built for through TG_VAR_COPY_LANES; odd lengths, two source pages"""
    import os
    r = np.random.default_rng(8)
    n = 1500
    key = Col("i32", r.integers(0, 50, n))
    assert "TG_VAR_COPY_LANES" not in os.environ
    for mean in (3, 30, 100, 400):
        lens = r.integers(0, 2 * mean + 1, n)
        blob = r.integers(0, 256, int(lens.sum()) + 1, dtype=np.uint8).tobytes()
        starts = np.concatenate([[0], np.cumsum(lens)])
        null = r.random(n) < 0.1
        pay = Col("str", [blob[starts[i]:starts[i + 1]] for i in range(n)], ~null)
        check(sess, ops, with_rid(key, pay), [0], [0], sizes=(700, 800))
        if mean != 30:
            continue
        try:
            for lanes in (1, 2, 4, 8, 16, 32, 64):
                os.environ["TG_VAR_COPY_LANES"] = str(lanes)
                check(sess, ops, with_rid(key, pay), [0], [0], sizes=(700, 800))
        finally:
            del os.environ["TG_VAR_COPY_LANES"]


# --------------------------------------------------------------------------
# topn_ex
# --------------------------------------------------------------------------
def test_topn_ex_limits(sess, ops):
    r = np.random.default_rng(3)
    n = 500
    pool = [b"", b"a", b"ab", b"abc" * 5, b"b"]
    null = r.random(n) < 0.1
    key = Col("str", [POISON_STR if z else pool[k] for z, k in zip(null, r.integers(0, 5, n))],
              ~null)
    cols = with_rid(key, Col("f64", r.standard_normal(n), r.random(n) >= 0.2))
    for desc in (0, 1):
        for limit in (1, n - 1, n, n + 1, 7, 50):          # 7 and 50 fall inside runs of ties
            rid = check(sess, ops, cols, [0], [desc], limit=limit)
            assert len(rid) == min(limit, n)
    assert check(sess, ops, slice_cols(cols, 0, 1), [0], [0], limit=5) == [0]


@pytest.mark.parametrize("n", [1000, 70_000])
def test_topn_ex_fixed_width_tie_order(sess, ops, n):
    """below and above the 65 536 rows at which tg_topn_create changes path:
    tg_topn_create_ex orders on the device at both and ties keep input order"""
    r = np.random.default_rng(n)
    cols = with_rid(Col("i64", r.integers(0, 5, n)), Col("f64", r.integers(0, 3, n) * 0.5))
    for limit in (n // 2, n):
        rid = check(sess, ops, cols, [0, 1], [1, 0], limit=limit)
        k0, k1 = cols[0].values[rid], cols[1].values[rid]
        same = (np.diff(k0) == 0) & (np.diff(k1) == 0)
        assert (np.diff(rid)[same] > 0).all() and same.sum() > limit // 2


# --------------------------------------------------------------------------
# against the Window operator
# --------------------------------------------------------------------------
def test_fixed_width_order_by_equals_window_row_order(sess, ops):
    r = np.random.default_rng(17)
    n = 5000
    fpool = np.array([0.0, -0.0, math.nan, 2.5, -1.0])
    cols = with_rid(Col("i64", r.integers(-4, 5, n), r.random(n) >= 0.1),
                    Col("f64", fpool[r.integers(0, 5, n)], r.random(n) >= 0.1))
    types = [tg_type(ops, c.kind) for c in cols]
    pages = split(cols, page_sizes(n))
    for desc in ([0, 0], [1, 0], [0, 1]):
        rid = check_pages(sess, ops, pages, [0, 1], desc)
        win = run_pages(ops.window(sess, types, [], [0, 1], desc,
                                   [(ops.WIN_ROW_NUMBER, -1, ops.WIN_FRAME_RANGE)]), ops, pages)
        assert win[0][2]["values"].tolist() == rid
        assert win[0][3]["values"].tolist() == list(range(1, n + 1))


# --------------------------------------------------------------------------
# ABI behaviour
# --------------------------------------------------------------------------
def raw_create(ops, sess, entry, types, sort, sort_desc, n_sort, out_ch=None, n_out=0, limit=5,
               null_session=False, null_types=False, null_out=False):
    """tg_order_by_create / tg_topn_create_ex with every pointer and count
    under the caller's control"""
    from trino_amd import _lib, _check
    ty = np.array(types, np.int32)
    arr = lambda v: None if v is None else np.array(v, np.int32)      # noqa: E731
    ptr = lambda a: None if a is None else a.ctypes.data              # noqa: E731
    sc, sd, oc = arr(sort), arr(sort_desc), arr(out_ch)
    h = ctypes.c_void_p()
    head = (None if null_session else sess._h, None if null_types else ty.ctypes.data, len(ty),
            ptr(sc), ptr(sd), n_sort)
    ref = None if null_out else ctypes.byref(h)
    if entry == "order_by":
        st = _lib.tg_order_by_create(*head, ptr(oc), n_out, ref)
    else:
        st = _lib.tg_topn_create_ex(*head, limit, ref)
    assert (st == 0) == bool(h.value)
    if h.value:
        _lib.tg_operator_close(h)
    _check(st)


@pytest.mark.parametrize("entry", ["order_by", "topn_ex"])
def test_rejections_by_status(sess, ops, entry):
    B, V = ops.TG_BIGINT, ops.TG_VARCHAR
    ok = dict(types=[V, B], sort=[0], sort_desc=[1], n_sort=1)
    raw_create(ops, sess, entry, **ok)                              # the base case is accepted
    inv = lambda **kw: expect_error(lambda: raw_create(ops, sess, entry, **{**ok, **kw}),  # noqa: E731
                                    TG_ERR_INVALID_ARG)
    inv(null_session=True)
    inv(null_types=True)
    inv(null_out=True)
    inv(n_sort=0)
    inv(n_sort=-1)
    inv(sort=None)                      # null arrays with a non-zero count
    inv(sort_desc=None)
    for ch in (-1, 2, 7):
        inv(sort=[ch])
        inv(sort=[0, ch], sort_desc=[0, 0], n_sort=2)
    if entry == "topn_ex":
        inv(limit=0)
        inv(limit=-3)
        raw_create(ops, sess, entry, **{**ok, "limit": 2 ** 31 - 1})
    else:
        inv(out_ch=None, n_out=1)
        inv(out_ch=[0], n_out=-1)
        for ch in (-1, 2, 7):
            inv(out_ch=[0, ch], n_out=2)
        raw_create(ops, sess, entry, **{**ok, "out_ch": [1, 1, 0], "n_out": 3})
        raw_create(ops, sess, entry, **{**ok, "out_ch": None, "n_out": 0})


@pytest.mark.parametrize("entry", ["order_by", "topn_ex"])
def test_page_shape_rejections_leave_the_operator_usable(sess, ops, entry):
    types = [ops.TG_VARCHAR, ops.TG_BIGINT, ops.TG_BIGINT]
    op = (ops.order_by(sess, types, [0], [0]) if entry == "order_by"
          else ops.topn_ex(sess, types, [0], [0], 10))
    try:
        s, i64, i32 = Col("str", [b"b", b"a"]), Col("i64", [1, 2]), Col("i32", [1, 2])
        rid = Col("i64", [0, 1])
        bad = lambda cols: expect_error(lambda: op.add_input(make_page(ops, cols)),   # noqa: E731
                                        TG_ERR_INVALID_ARG, entry)
        bad([s, i64])                   # fewer channels than declared
        bad([s, i32, rid])              # a narrower cell than declared
        bad([i64, i64, rid])            # fixed width where VARCHAR was declared
        bad([s, s, rid])                # VARCHAR where a fixed width was declared
        op.add_input(make_page(ops, [s, i64, rid]))
        out = op.drain()
        assert out[0][0]["values"] == [b"a", b"b"] and out[0][2]["values"].tolist() == [1, 0]
    finally:
        op.close()
    op = ops.order_by(sess, types, [0], [0])      # closable straight after a rejection
    expect_error(lambda: op.add_input(make_page(ops, [i64, i64, rid])), TG_ERR_INVALID_ARG)
    op.close()


def test_accumulated_bytes_and_rows_beyond_int32(sess, ops):
    """host-side sums at add_input: the second 2^30-byte string in a channel,
    and the second 2^30-row page, are refused before they are uploaded"""
    big = 1 << 30
    data = np.zeros(big, np.uint8)
    offs = np.array([0, big], np.int32)
    op = ops.order_by(sess, [ops.TG_BIGINT, ops.TG_VARCHAR], [0], [0])
    try:
        page = ops.page_with_varchar([np.array([1], np.int64), (data, offs)])
        op.add_input(page)
        expect_error(lambda: op.add_input(page), TG_ERR_UNSUPPORTED, "INT32_MAX bytes")
    finally:
        op.close()
    op = ops.topn_ex(sess, [ops.TG_TINYINT], [0], [0], 1)
    try:
        page = ops.page_from_numpy([data.view(np.int8)])
        op.add_input(page)
        expect_error(lambda: op.add_input(page), TG_ERR_UNSUPPORTED, "INT32_MAX rows")
    finally:
        op.close()
