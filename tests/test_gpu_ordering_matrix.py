"""Ordering parity matrix: the TopN operator (trino_amd/csrc/ops_topn.hip,
host partial_sort path and device radix path) and the page partitioner
(ops_partition.hip, with run_gather / run_gather_var of ops_filter.hip as
its second caller) against references written here.

TopN reference: Python `sorted` over per-row key tuples (topn_sort_key).
ASC puts NULLs last, DESC puts NULLs first. DOUBLE keys compare numerically
with -0.0 == +0.0, and every NaN (either sign bit, any payload) ranks as the
single largest non-NULL value, Trino's ORDER BY rule (include/trino_gpu.h).
Order among rows whose WHOLE sort key ties is unspecified (the host path's
partial_sort is unstable), so a case asserts
  (a) the output's sequence of key tuples equals the reference's under those
      equivalences (canon_key: NULL, one NaN, one zero), and
  (b) through a unique BIGINT row-id payload channel: the output rows are
      distinct input rows, and every channel of every output row equals that
      input row bit for bit, validity included.
Every NULL cell carries a poison value that would sort first if it were read.

Partitioner reference: oracle.hash_rows + oracle.partition_remote (the CPU
oracle tests/test_oracle_units.py pins to public vectors); the stable split
is plain Python. NULL partition keys are out of scope: the operator's header
says so and the oracle wrapper passes no validity.

Host-side checks of the references and shapes are in
tests/test_oracle_units.py::TestOrderingMatrixHost (no GPU).
"""
import functools
import math
import os
import re

import numpy as np
import pytest

from test_gpu_filter_matrix import (Col, KINDS, _NP, expect_error, make_page, tg_type,
                                    unpack_bits, TG_ERR_INVALID_ARG, TG_ERR_UNSUPPORTED)

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "trino_amd", "csrc")


@functools.lru_cache(None)
def source_constants():
    topn = open(os.path.join(_CSRC, "ops_topn.hip")).read()
    part = open(os.path.join(_CSRC, "ops_partition.hip")).read()

    def one(pat, text):
        m = re.search(pat, text)
        assert m, pat
        return int(m.group(1))

    return dict(
        TOPN_DEVICE_ROWS=one(r"return total_rows >= (\d+);", topn),
        PCHUNK=one(r"#define PCHUNK (\d+)", part),
        MAX_PARTS=one(r"partition_count > (\d+)", part),
        RETIRED=one(r"retired_\.size\(\) > (\d+)", part),
    )


# assumed by the shapes; TestOrderingMatrixHost pins them to the parsed values
TOPN_DEVICE_ROWS = 65536
PCHUNK = 16384
MAX_PARTS = 256
HOST_ROWS = 1000

PATH_ROWS = {"host": HOST_ROWS, "device": TOPN_DEVICE_ROWS}


def page_sizes(rows):
    """1, 0, rows - 2 and 1 rows: a total of exactly `rows`"""
    return (1, 0, rows - 2, 1) if rows >= 2 else (rows,)


PART_SIZES = (0, 1, 64, 65, PCHUNK - 1, PCHUNK, PCHUNK + 1, 2 * PCHUNK + 1)
PART_COUNTS = (1, 2, 63, 64, 65, MAX_PARTS)


def partition_shapes():
    return [(n, p) for p in PART_COUNTS for n in PART_SIZES]


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
# TopN reference
# --------------------------------------------------------------------------
def _is_nan(v):
    return isinstance(v, float) and v != v


def topn_sort_key(key, desc):
    """sortable tuple of one row's sort-key cells (None = NULL)"""
    out = []
    for v, d in zip(key, desc):
        if v is None:
            out.append((0, 0, 0) if d else (1, 0, 0))     # DESC first, ASC last
        elif _is_nan(v):
            out.append((1, 0, 0) if d else (0, 1, 0))     # the largest value
        else:
            out.append((1, 1, -v) if d else (0, 0, v))    # -0.0 == 0.0 either way
    return tuple(out)


def canon_key(key):
    """NULL, one NaN and one zero: the equivalences of the contract"""
    return tuple(None if v is None else "nan" if _is_nan(v) else
                 (v + 0.0 if isinstance(v, float) else v) for v in key)


def ref_topn(keys, desc, limit):
    """row indices of the top `limit` rows in output order (ties among equal
    whole keys in input order, which the comparison does not rely on)"""
    order = sorted(range(len(keys)), key=lambda i: topn_sort_key(keys[i], desc))
    return order[:limit]


# --------------------------------------------------------------------------
# TopN runner
# --------------------------------------------------------------------------
def cells(col):
    vals = col.values.tolist()
    if col.valid is None:
        return vals
    return [v if ok else None for v, ok in zip(vals, col.valid.tolist())]


def slice_cols(cols, lo, hi):
    return [Col(c.kind, c.values[lo:hi], None if c.valid is None else c.valid[lo:hi])
            for c in cols]


def run_topn(sess, ops, cols, sort_channels, desc, limit, sizes):
    op = ops.topn(sess, [tg_type(ops, c.kind) for c in cols], sort_channels, desc, limit)
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


def check_topn(sess, ops, cols, sort_channels, desc, limit, sizes=None):
    """cols: the LAST column is the unique BIGINT row id"""
    n = len(cols[0])
    sizes = page_sizes(n) if sizes is None else sizes
    pages = run_topn(sess, ops, cols, sort_channels, desc, limit, sizes)
    take = min(limit, n)
    if n == 0:
        assert all(len(p[0]["values"]) == 0 for p in pages)
        return
    assert len(pages) == 1 and len(pages[0]) == len(cols)
    out = pages[0]
    rid = np.asarray(out[-1]["values"], np.int64)
    assert len(rid) == take, (len(rid), take)
    assert unpack_bits(out[-1]["valid"], take).all()
    # (b) distinct input rows, every channel equal, validity included
    assert ((rid >= 0) & (rid < n)).all() and len(np.unique(rid)) == take
    got_cols = []
    for c, src in enumerate(cols):
        assert out[c]["type"] == tg_type(ops, src.kind), (c, out[c]["type"])
        g = np.asarray(out[c]["values"])
        gvalid = unpack_bits(out[c]["valid"], take)
        svalid = np.ones(n, bool) if src.valid is None else src.valid
        assert np.array_equal(gvalid, svalid[rid]), f"channel {c}: validity"
        view = np.int64 if src.kind == "f64" else _NP[src.kind]
        bad = np.flatnonzero((g.view(view) != src.values[rid].view(view)) & gvalid)
        assert len(bad) == 0, f"channel {c}: output row {bad[0]} is not input row {rid[bad[0]]}"
        got_cols.append(Col(src.kind, g, gvalid))
    # (a) the key sequence, from the output's own cells
    key_cells = [cells(cols[c]) for c in sort_channels]
    keys = list(zip(*key_cells))
    exp = [canon_key(keys[i]) for i in ref_topn(keys, desc, limit)]
    got = [canon_key(k) for k in zip(*[cells(got_cols[c]) for c in sort_channels])]
    if got != exp:
        k = next(i for i, (a, b) in enumerate(zip(got, exp)) if a != b)
        raise AssertionError(f"key sequence differs at output {k}: got {got[k]} "
                             f"expected {exp[k]}")


def key_col(kind, n, seed, null_share, desc, distinct=None):
    """random key column; NULL cells hold the value that would sort FIRST"""
    r = np.random.default_rng(seed)
    info = None if kind == "f64" else np.iinfo(_NP[kind])
    if kind == "f64":
        vals = np.round(r.standard_normal(n) * 1000) / 8
    elif kind == "bool":
        vals = r.integers(0, 2, n)
    else:
        lo, hi = max(info.min, -2 ** 40), min(info.max, 2 ** 40)
        vals = r.integers(lo, hi, n, endpoint=True)
    if distinct:
        pool = vals[:distinct]
        vals = pool[r.integers(0, distinct, n)]
    vals = np.asarray(vals, _NP[kind])
    if not null_share:
        return Col(kind, vals)
    null = r.random(n) < null_share
    if kind == "f64":
        vals[null] = math.inf if desc else -math.inf
    elif kind == "bool":
        vals[null] = 1 if desc else 0
    else:
        vals[null] = info.max if desc else info.min
    return Col(kind, vals, ~null)


def payload_cols(n, seed):
    """a nullable DOUBLE and SMALLINT payload and the unique row id (last):
    the row's position in the concatenated input"""
    r = np.random.default_rng(seed)
    return [Col("f64", r.standard_normal(n), r.random(n) >= 0.2),
            Col("i16", r.integers(-30000, 30000, n), r.random(n) >= 0.5),
            Col("i64", np.arange(n))]


PATHS = ("host", "device")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("desc", [0, 1], ids=["asc", "desc"])
@pytest.mark.parametrize("kind", KINDS)
def test_topn_single_key_every_type(sess, ops, kind, desc, path):
    """k_topn_keys / topn_sortable per type (device), the typed host
    comparator (host); 10 % NULL keys, NULLs in both payloads (T1)"""
    n = PATH_ROWS[path]
    cols = [key_col(kind, n, 1, 0.1, desc)] + payload_cols(n, 2)
    check_topn(sess, ops, cols, [0], [desc], 25)


MULTI = (([0, 1], [0, 1]), ([0, 1], [1, 0]), ([1, 0], [1, 1]),
         ([0, 1, 2], [0, 1, 0]), ([2, 0, 1], [1, 0, 1]), ([1, 2, 0], [0, 0, 0]))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("channels,desc", MULTI, ids=[f"{c}{d}".replace(" ", "") for c, d in MULTI])
def test_topn_multi_channel_heavy_ties(sess, ops, channels, desc, path):
    """2 and 3 sort channels, mixed directions; the leading keys take 7
    distinct values, so the LSD passes (device) and the channel loop of the
    comparator (host) decide most positions on a later channel"""
    n = PATH_ROWS[path]
    cols = [key_col("i32", n, 3, 0.1, desc[channels.index(0)], distinct=7),
            key_col("f64", n, 4, 0.1, desc[channels.index(1)], distinct=7),
            key_col("i64", n, 5, 0.1, 0, distinct=7)] + payload_cols(n, 6)
    check_topn(sess, ops, cols, channels, desc, 300)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("limit", ["1", "25", "rows", "rows+5"])
def test_topn_limits(sess, ops, limit, path):
    n = PATH_ROWS[path]
    lim = {"1": 1, "25": 25, "rows": n, "rows+5": n + 5}[limit]
    cols = [key_col("i64", n, 7, 0.1, 1), key_col("f64", n, 8, 0.1, 0)] + payload_cols(n, 9)
    check_topn(sess, ops, cols, [0, 1], [1, 0], lim)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("desc", [0, 1], ids=["asc", "desc"])
def test_topn_all_null_key(sess, ops, desc, path):
    """a leading key that is NULL in every row: the second channel decides"""
    n = PATH_ROWS[path]
    allnull = Col("i64", np.full(n, 5), np.zeros(n, bool))
    cols = [allnull, key_col("i32", n, 10, 0.1, desc)] + payload_cols(n, 11)
    check_topn(sess, ops, cols, [0, 1], [desc, desc], 40)


def test_topn_zero_rows(sess, ops):
    cols = [key_col("i64", 0, 1, 0, 0)] + payload_cols(0, 2)
    check_topn(sess, ops, cols, [0], [0], 10, sizes=(0, 0))
    check_topn(sess, ops, cols, [0], [1], 10, sizes=())


def special_cols(name, n, seed):
    r = np.random.default_rng(seed)
    null = r.random(n) < 0.25
    if name == "int64_extremes":          # T2: INT64_MAX's image was the sentinel
        pool = np.array([-2 ** 63, 2 ** 63 - 1, -2 ** 63 + 1, 2 ** 63 - 2, 0, -1], np.int64)
        return Col("i64", pool[r.integers(0, len(pool), n)], ~null)
    if name == "double_specials":         # T3
        pool = np.array([0.0, -0.0, math.inf, -math.inf, 1.5, -1.5, 5e-324, -5e-324],
                        np.float64)
        vals = pool[r.integers(0, len(pool), n)]
        nan_bits = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001,
                             0xFFF0000000000001, 0xFFFFFFFFFFFFFFFF], np.uint64)
        nan = r.random(n) < 0.3
        vals = np.where(nan, nan_bits[r.integers(0, len(nan_bits), n)].view(np.float64), vals)
        return Col("f64", vals, ~null)
    if name == "all_ones_nan":            # the DOUBLE whose bits were the sentinel
        pool = np.array([0x7FFFFFFFFFFFFFFF, 0x7FF0000000000000, 0x7FEFFFFFFFFFFFFF,
                         0x0000000000000000], np.uint64).view(np.float64)
        return Col("f64", pool[r.integers(0, len(pool), n)], ~null)
    raise ValueError(name)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("desc", [0, 1], ids=["asc", "desc"])
@pytest.mark.parametrize("name", ["int64_extremes", "double_specials", "all_ones_nan"])
def test_topn_special_keys(sess, ops, name, desc, path):
    """limit == rows, so the whole order is checked: values, the NaN group,
    the NULL group, and a second key that orders inside each of them"""
    n = PATH_ROWS[path]
    cols = [special_cols(name, n, 12), key_col("i32", n, 13, 0, 0)] + payload_cols(n, 14)
    check_topn(sess, ops, cols, [0, 1], [desc, 0], n)


@pytest.mark.parametrize("desc", [0, 1], ids=["asc", "desc"])
def test_topn_path_switch(sess, ops, desc):
    """threshold - 1 rows (host) and the same data plus one appended row
    (device): both satisfy the contract"""
    n = TOPN_DEVICE_ROWS
    cols = [special_cols("double_specials", n, 15), key_col("i64", n, 16, 0.1, 0, distinct=50)]
    cols += payload_cols(n, 17)               # ids are positions: a prefix keeps them dense
    check_topn(sess, ops, slice_cols(cols, 0, n - 1), [0, 1], [desc, 1 - desc], 500)
    check_topn(sess, ops, cols, [0, 1], [desc, 1 - desc], 500)


def test_topn_rejects_varchar_and_bad_specs(sess, ops):
    """T4: no plan puts a VARCHAR channel through TopN, and the output gather
    moves fixed-width cells only, so tg_topn_create refuses it"""
    for types in ([ops.TG_VARCHAR], [ops.TG_BIGINT, ops.TG_VARCHAR]):
        expect_error(lambda: ops.topn(sess, types, [0], [0], 5), TG_ERR_UNSUPPORTED, "VARCHAR")
    for ch in (-1, 1, 7):
        expect_error(lambda: ops.topn(sess, [ops.TG_BIGINT], [ch], [0], 5),
                     TG_ERR_INVALID_ARG, "sort channel")
    expect_error(lambda: ops.topn(sess, [ops.TG_BIGINT], [0], [0], 0), TG_ERR_INVALID_ARG)
    op = ops.topn(sess, [ops.TG_BIGINT, ops.TG_BIGINT], [0], [0], 5)
    try:
        narrow = [Col("i64", [1, 2]), Col("i32", [1, 2])]
        expect_error(lambda: op.add_input(make_page(ops, narrow)), TG_ERR_INVALID_ARG, "topn")
        expect_error(lambda: op.add_input(make_page(ops, narrow[:1])), TG_ERR_INVALID_ARG, "topn")
    finally:
        op.close()


# --------------------------------------------------------------------------
# partitioner
# --------------------------------------------------------------------------
_ORACLE_TYPE = {"i64": 0, "i32": 1, "i16": 2, "i8": 3, "f64": 4, "date": 5, "bool": 6}


def ref_partition_ids(key_cols, nparts):
    import oracle
    hashes = oracle.hash_rows([c.values for c in key_cols],
                              [_ORACLE_TYPE[c.kind] for c in key_cols])
    memo, out = {}, np.empty(len(hashes), np.int32)
    for i, h in enumerate(hashes.view(np.int64).tolist()):
        p = memo.get(h)
        if p is None:
            p = memo[h] = oracle.partition_remote(h, nparts)
        out[i] = p
    return out


def ref_split(pids, nparts):
    """stable split: the rows of each partition in input order"""
    out = [[] for _ in range(nparts)]
    for i, p in enumerate(pids.tolist()):
        out[p].append(i)
    return out


def assert_partition_page(ops, got, cols, rows, what):
    if got is None:
        assert len(rows) == 0, f"{what}: empty page, {len(rows)} rows expected"
        return
    rows = np.array(rows, np.int64)
    assert len(got) == len(cols)
    for c, src in enumerate(cols):
        assert got[c]["type"] == tg_type(ops, src.kind), (what, c)
        n = len(rows)
        gvalid = unpack_bits(got[c]["valid"], n)
        svalid = np.ones(len(src), bool) if src.valid is None else src.valid
        assert len(got[c]["values"]) == n, (what, c, len(got[c]["values"]), n)
        assert np.array_equal(gvalid, svalid[rows]), f"{what}: channel {c} validity"
        if src.kind == "str":
            exp = [src.values[i] if svalid[i] else b"" for i in rows]
            assert got[c]["values"] == exp, f"{what}: channel {c} bytes"
            offs = got[c]["offsets"].astype(np.int64)
            assert offs[0] == 0 and np.array_equal(np.diff(offs), [len(x) for x in exp])
            continue
        view = np.int64 if src.kind == "f64" else _NP[src.kind]
        g = np.asarray(got[c]["values"])
        bad = np.flatnonzero((g.view(view) != src.values[rows].view(view)) & gvalid)
        assert len(bad) == 0, f"{what}: channel {c} differs at output row {bad[0]}"


def check_partitioner(sess, ops, pages, key_channels, nparts):
    """all pages in, then every partition fetched oldest-first and downloaded
    at fetch time; one more fetch per partition returns the empty page"""
    types = [tg_type(ops, c.kind) for c in pages[0]]
    op = ops.page_partitioner(sess, types, key_channels, nparts)
    try:
        for cols in pages:
            op.add_input(make_page(ops, cols))
        op.finish()
        splits = [ref_split(ref_partition_ids([cols[k] for k in key_channels], nparts), nparts)
                  for cols in pages]
        for p in range(nparts):
            for j, cols in enumerate(pages):
                got = ops.get_partition(sess, op, p)
                assert_partition_page(ops, got, cols, splits[j][p], f"partition {p} page {j}")
            assert ops.get_partition(sess, op, p) is None
    finally:
        op.close()
    return splits


def part_cols(n, seed, distinct=4096):
    r = np.random.default_rng(seed)
    pool = r.integers(-2 ** 62, 2 ** 62, distinct)
    return [Col("i64", pool[r.integers(0, distinct, n)] if n else np.empty(0, np.int64)),
            Col("i32", np.arange(n), r.random(n) >= 0.1)]


@pytest.mark.parametrize("nparts", PART_COUNTS)
def test_partitioner_sizes(sess, ops, nparts):
    """k_partition_ids, k_part_count, k_part_scan, k_part_scatter (its
    64-lane loop over partitions at 63 / 64 / 65 / 256) and k_gather at every
    size edge of PCHUNK"""
    for n in PART_SIZES:
        splits = check_partitioner(sess, ops, [part_cols(n, n + nparts)], [0], nparts)
        if n >= PCHUNK and nparts <= 65:
            assert all(len(rows) for rows in splits[0])      # every partition is used


@pytest.mark.parametrize("nparts", [1, 64, 65, MAX_PARTS])
def test_partitioner_skews(sess, ops, nparts):
    import oracle
    n = PCHUNK + 65
    const = [Col("i64", np.full(n, 424242)), Col("i32", np.arange(n))]
    splits = check_partitioner(sess, ops, [const], [0], nparts)
    assert sorted(len(r) for r in splits[0])[-1] == n        # one partition takes all
    keys, seen, k = [], set(), 0
    while len(seen) < nparts:                                # one row per partition
        h = int(oracle.hash_rows([np.array([k], np.int64)], [0]).view(np.int64)[0])
        p = oracle.partition_remote(h, nparts)
        if p not in seen:
            seen.add(p)
            keys.append(k)
        k += 1
    one = [Col("i64", keys), Col("i32", np.arange(nparts))]
    splits = check_partitioner(sess, ops, [one], [0], nparts)
    assert all(len(r) == 1 for r in splits[0])


def wide_pages(sizes, seed):
    """two-channel key (INTEGER, DOUBLE with -0.0), payloads of every width
    with NULLs, and a VARCHAR payload with NULLs and empty strings"""
    r = np.random.default_rng(seed)
    words = [b"", b"a", b"partition", b"", b"x" * 70]
    pages = []
    for n in sizes:
        fpool = np.array([0.0, -0.0, 1.5, -2.25, 1e300, 3.0])
        cols = [Col("i32", r.integers(-5, 6, n)), Col("f64", fpool[r.integers(0, 6, n)])]
        for kind in KINDS:
            info = None if kind == "f64" else np.iinfo(_NP[kind])
            vals = (r.standard_normal(n) if kind == "f64" else r.integers(0, 2, n)
                    if kind == "bool" else r.integers(info.min, info.max, n, endpoint=True))
            cols.append(Col(kind, vals, r.random(n) >= 0.15))
        null = r.random(n) < 0.15
        strs = [b"<poison>" if z else words[k] for z, k in zip(null, r.integers(0, 5, n))]
        cols.append(Col("str", strs, ~null))
        cols.append(Col("str", [b"%d" % i for i in range(n)]))
        pages.append(cols)
    return pages


@pytest.mark.parametrize("nparts", [2, 7, 65])
def test_partitioner_wide_rows_three_pages(sess, ops, nparts):
    """run_gather at every width and run_gather_var from the partitioner;
    three input pages per partition against a retired window of two"""
    pages = wide_pages((PCHUNK + 3, 0, 700), nparts)
    check_partitioner(sess, ops, pages, [0, 1], nparts)


def test_partitioner_negative_zero_key_hashes_like_the_oracle(sess, ops):
    n = 512
    cols = [Col("f64", np.where(np.arange(n) % 2 == 0, 0.0, -0.0)), Col("i32", np.arange(n))]
    check_partitioner(sess, ops, [cols], [0], 64)


def test_partitioner_rejections(sess, ops):
    for nparts in (0, -1, MAX_PARTS + 1):
        expect_error(lambda: ops.page_partitioner(sess, [ops.TG_BIGINT], [0], nparts),
                     TG_ERR_INVALID_ARG, "partition")
    op = ops.page_partitioner(sess, [ops.TG_BIGINT], [0], 5)
    try:
        op.add_input(make_page(ops, [Col("i64", np.arange(100))]))
        for p in (-1, 5, 6):
            expect_error(lambda: ops.get_partition(sess, op, p), TG_ERR_INVALID_ARG,
                         "bad partition")
    finally:
        op.close()
