"""Pool balance of the ordering path and of the hash join: TopN (both paths),
Window, tg_dedup_i64 and the join's build, probe, lookup-outer and semi
operators return every temporary to the session pool.

Each case records live = total - cached pool bytes (trino_amd.session_memory)
before the operator exists, runs it to completion, closes it and expects
exactly that value again; `live` and not `total`, because the pool may evict
cached buffers. Each case also compares the output with a reference
(np.lexsort, ref_window_ex_vec of test_window_frames_reference, np.unique,
ref_join / ref_semi / ref_unmatched through the join matrices' runners), so
none passes by doing nothing. The shapes are the smallest at which every
temporary of the path is taken. The failure paths need an allocation failure
and are not run here.
"""
import numpy as np
import pytest

import test_gpu_join_matrix as jm
from test_gpu_filter_matrix import Col, POISON, unpack_bits
from test_gpu_join_matrix import partitioned  # noqa: F401  (fixture)
from test_gpu_ordering_matrix import HOST_ROWS, TOPN_DEVICE_ROWS, run_topn
from test_gpu_outer_join_matrix import single_key_outer
from test_gpu_text_distinct_matrix import run_dedup
from test_gpu_window_frames_matrix import check_window_ex
from test_gpu_window_matrix import WSCAN_ONE_WAVE
from test_window_frames_reference import LAG, ROWS_BETWEEN, ex
from test_window_reference import MIN_I64, RANGE, ROW_NUMBER, SUM_I64

pytestmark = pytest.mark.gpu

TOPN_LIMIT = 10


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


def live(sess):
    from trino_amd import session_memory
    total, cached = session_memory(sess)
    return total - cached


def topn_cols(n):
    """[nullable key of 7 values, unique key, row id]: no two whole keys tie"""
    r = np.random.default_rng(n)
    present = r.random(n) >= 0.25
    a = r.integers(-3, 4, n)
    a[~present] = POISON["i64"]
    return [Col("i64", a, present), Col("i64", r.permutation(n)), Col("i64", np.arange(n))]


@pytest.mark.parametrize("rows", [TOPN_DEVICE_ROWS, HOST_ROWS], ids=["device", "host"])
def test_topn(sess, ops, rows):
    """ORDER BY a DESC (nulls first), b ASC LIMIT 10 over pages of
    (1, 0, rows - 3, 2) rows: the null pass of `a` runs on the device path"""
    cols = topn_cols(rows)
    a, b = cols[0], cols[1]
    # least significant key first; NULL before every value, then a descending
    exp = np.lexsort((b.values, np.where(a.valid, -a.values, 0), a.valid))[:TOPN_LIMIT]
    start = live(sess)
    pages = run_topn(sess, ops, cols, [0, 1], [1, 0], TOPN_LIMIT, (1, 0, rows - 3, 2))
    assert live(sess) == start
    assert len(pages) == 1 and len(pages[0]) == 3
    out = pages[0]
    assert np.array_equal(np.asarray(out[2]["values"], np.int64), exp)
    valid = unpack_bits(out[0]["valid"], TOPN_LIMIT)
    assert np.array_equal(valid, a.valid[exp])
    assert np.array_equal(np.asarray(out[0]["values"])[valid], a.values[exp][valid])
    assert np.array_equal(np.asarray(out[1]["values"]), b.values[exp])


def test_window(sess, ops):
    """one row more than a wave scans alone, so the carry arrays are taken;
    the bounded MIN frame takes the sparse-table buffers"""
    n = WSCAN_ONE_WAVE + 1
    r = np.random.default_rng(7)
    part_present, x_present = r.random(n) >= 0.2, r.random(n) >= 0.3
    part = r.integers(0, 9, n)
    part[~part_present] = POISON["i64"]
    x = r.integers(-10 ** 12, 10 ** 12, n)
    x[~x_present] = POISON["i64"]
    cols = [Col("i64", part, part_present), Col("i64", r.permutation(n)),
            Col("i64", x, x_present), Col("i64", np.arange(n))]
    specs = [ex(ROW_NUMBER), ex(SUM_I64, 2, RANGE), ex(MIN_I64, 2, ROWS_BETWEEN, -3, 3),
             ex(LAG, 2, offset=1)]
    start = live(sess)
    assert check_window_ex(sess, ops, cols, [0], [1], [0], specs) is not None
    assert live(sess) == start


def test_dedup(sess, ops):
    keys = np.random.default_rng(11).integers(0, 100, 1000).astype(np.int64)
    exp = np.unique(keys)
    start = live(sess)
    m, got = run_dedup(sess, keys, 64)
    assert live(sess) == start
    assert m == len(exp) and np.array_equal(got, exp)


# --------------------------------------------------------------------------
# hash join: build, probe paths, lookup-outer and semi join. Each case is a
# checked case of the join matrices, which compare every column against
# ref_join, ref_semi or ref_unmatched and close the operators and the bridge.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("outer", [False, True], ids=["inner", "outer"])
def test_join_csr_classic(sess, ops, outer):
    """nullable key bitmap, the CSR temporaries, count / scan / fill and the
    gathers (with NULL positions when probe-outer)"""
    start = live(sess)
    jm.single_key_case(sess, ops, "nulls", 1000, jm.SMALL_M, outer)
    assert live(sess) == start


def test_join_multi_page_varchar(sess, ops):
    """VARCHAR concatenation, the generic build key columns and the probe-side
    key column array"""
    start = live(sess)
    jm.multi_page_varchar_case(sess, ops, False)
    assert live(sess) == start


def test_join_partitioned_overflow_retry(sess, ops, partitioned):  # noqa: F811
    """the six partition temporaries, the early release of the first-try match
    lists and the match sort"""
    build, probe = jm.bigint_tables(*jm.overflow_inputs())
    start = live(sess)
    got = jm.join_case(sess, ops, [build], [0], [0, 1, 2], [probe], [0], [0, 1],
                       False, order="list")
    assert live(sess) == start
    assert len(got[0]) == jm.OVERFLOW_N * jm.OVERFLOW_N


def test_join_full_and_lookup_outer(sess, ops):
    """the visited bitmap, the unmatched-row emission and its all-NULL columns"""
    start = live(sess)
    assert single_key_outer(sess, ops, "dups", 1000, jm.SMALL_M, 3) is not None
    assert live(sess) == start


def test_semi_join_set_source(sess, ops):
    """set builder over a dense key range: the bitmap and no index"""
    bk, bnull = jm.set_shapes()["nulls_inside_run"]
    lo, hi = int(bk.min()), int(bk.max())
    pk = np.arange(lo - 70, hi + 71, dtype=np.int64)
    build = [jm.nullable("i64", bk, bnull, lo - 3)]
    probe = [jm.nullable("i64", pk, np.arange(len(pk)) % 13 == 6, lo)]
    start = live(sess)
    jm.semi_case(sess, ops, [build], 0, [probe], 0, source="set")
    assert live(sess) == start


def test_semi_join_generic_key(sess, ops):
    """a DOUBLE key takes the generic path and the probe-side key column array"""
    build, probe = jm.semi_tables("double", "dups", True)
    start = live(sess)
    jm.semi_case(sess, ops, [build], 0, [probe], 0, source="hash")
    assert live(sess) == start


def test_join_requested_bitmap(sess, ops):
    """a dynamic-filter bitmap requested beside the index; these sparse keys
    span more than 2^33, so only the key-range pass runs"""
    start = live(sess)
    jm.single_key_case(sess, ops, "unique", 1000, jm.SMALL_M, False,
                       request_bitmap=True)
    assert live(sess) == start


def test_join_requested_bitmap_dense(sess, ops):
    """the same over a dense key range, where the bitmap is built"""
    r = np.random.default_rng(12)
    bk = r.integers(-300, 900, 1000).astype(np.int64)
    pk = r.integers(-400, 1000, jm.SMALL_M).astype(np.int64)
    build, probe = jm.bigint_tables(bk, np.arange(1000) % 50 == 7, pk, None)
    start = live(sess)
    jm.join_case(sess, ops, [build], [0], [0, 1, 2], [probe], [0], [0, 1], False,
                 request_bitmap=True)
    assert live(sess) == start
