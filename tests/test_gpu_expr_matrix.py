"""IS_NULL, SELECT, COALESCE, the NULL literal and IN lists on the device,
bit-exact against tests/test_expr_reference.py::ref_eval2, through every
entry that takes a tg_expr: tg_filter_run (whole page, range and list
selections, dictionary blocks), FilterProjectOp (BIGINT and DOUBLE outputs,
with the dynamic filter, fused under TG_FP_FUSED=1 in a child process) and the
lookup join's residual filter.

Selection vectors are compared in order; projections by bits and validity
with the NaN rule of test_gpu_filter_matrix. Every NULL cell carries a poison
value. Pages are the seven-type page of the filter matrix at 1031 rows unless
a test is about the row count.

The set term of k_filter_terms has three forms (one-word mask, device bitmap,
sorted array); path_of2 of the reference file says which kernel a program
takes and in_form which form, so each case states the ground it stands on.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_join_filter_matrix as jfm
from test_expr_reference import (IN_BITMAP_BITS, IN_LIST_MAX, FORM_BITMAP, FORM_MASK,
                                 FORM_SEARCH, N_PROGRAMS, case_chain, in_form, path_of2,
                                 random_case, random_rows, ref_eval2, ref_keep2)
from test_gpu_filter_matrix import (CHUNK, FTERM_MAX, GRID_N, GRID_THREADS, I64_MAX, I64_MIN,
                                    KINDS, N_TYPED, PERIOD, POISON, Col, _NP,
                                    assert_projection, chain, df_bridge, dict_case, dict_page,
                                    expect_error, grid_cols, make_page, rows_of, selection,
                                    seven_page, tg_type, tiled, unpack_bits)
from test_gpu_filter_matrix import ops, sess  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TG_ERR_UNSUPPORTED = 6

C = lambda i: ("col", i)           # noqa: E731
I = lambda v: ("i64", v)           # noqa: E731
F = lambda v: ("f64", v)           # noqa: E731
NULL = lambda lane: ("null", lane)  # noqa: E731
IN = lambda *v: ("in", list(v))    # noqa: E731


# --------------------------------------------------------------------------
# runners
# --------------------------------------------------------------------------
def kinds_of(cols):
    return tuple(c.kind for c in cols)


def check_filter(sess, ops, cols, prog, sel=None, rows=None, page=None, path=None):
    kinds = kinds_of(cols)
    if path is not None:
        assert path_of2(prog, kinds) == path, (path_of2(prog, kinds), prog)
    rows = rows_of(cols) if rows is None else rows
    page = make_page(ops, cols) if page is None else page
    tsel, positions = (None, range(len(rows))) if sel is None else selection(ops, *sel)
    got = ops.filter_run(sess, ops.expr(*prog), page, tsel)
    exp = [i for i in positions if ref_keep2(prog, rows[i], kinds)]
    assert got.tolist() == exp, (prog, len(got), len(exp))


def check_project(sess, ops, cols, filt, projs, make_op=None, keep=None):
    """projs: (prog, 'i64' | 'f64'); one page through one operator"""
    kinds = kinds_of(cols)
    out_types = [tg_type(ops, k) for _, k in projs]
    f = ops.expr(*filt) if filt is not None else None
    pe = [ops.expr(*p) for p, _ in projs]
    op = make_op(f, pe, out_types) if make_op else ops.filter_project(sess, f, pe, out_types)
    try:
        op.add_input(make_page(ops, cols))
        out = op.drain()[0]
    finally:
        op.close()
    rows = rows_of(cols)
    positions = [i for i in range(len(rows))
                 if (filt is None or ref_keep2(filt, rows[i], kinds)) and
                 (keep is None or keep(rows[i]))]
    for j, (prog, kind) in enumerate(projs):
        vals, valid = [], []
        for i in positions:
            v = ref_eval2(prog, rows[i], kinds)
            valid.append(not v[2])
            vals.append(0 if v[2] else (v[0] if v[1] else int(v[0])) if kind == "i64"
                        else 0.0 if v[2] else float(v[0]))
        assert out[j]["type"] == tg_type(ops, kind)
        assert_projection(out[j], vals, valid, kind, prog)
    return out


# columns of seven_page: 0 i64, 1 i32, 2 date, 3 i16, 4 i8, 5 bool, 6 f64
SIZES = (49, 14, 23, 45, 19, 3, 36, 9)
FILTERS = {
    "is_null": (C(6), "is_null"),
    "is_not_null_and": (C(0), "is_null", "not", C(1), I(0), "gt", "and"),
    "select": (C(1), C(0), I(0), "gt", C(3), "select", I(10), "gt"),
    "select_mixed_lanes": (C(0), C(5), C(6), "select", F(0.5), "ge"),
    "select_null_cond": (C(1), C(0), C(4), "lt", C(2), "select", I(0), "lt"),
    "coalesce_lane": (C(6), I(1), "coalesce", I(2), "div", F(0.5), "eq"),
    "coalesce_ints": (C(0), C(1), "coalesce", I(2), "div", I(0), "eq"),
    "null_or": (C(0), I(0), "gt", NULL(0), "or"),
    "null_double_lane": (NULL(1), C(3), "coalesce", I(7), "div", F(100.0), "gt"),
    "in_term": (C(1), IN(*SIZES)),
    "in_double_column": (C(6), IN(-3, 0, 25, 50)),
    "in_expression": (C(1), C(4), "add", IN(0, -7, 12, 150, -150)),
    "not_in": (C(3), IN(*range(-3000, 3001, 7)), "not"),
    "in_or_null": (C(4), IN(1, 2, 3), NULL(0), "or", "is_null"),
    "case_5_whens": case_chain(5) + (I(20), "ge"),
    "nullif": (C(1), C(1), C(4), "eq", NULL(0), "select", "is_null"),
    "if_in": (C(0), C(2), IN(1, 5, -9, 60), C(3), "select", C(1), "gt"),
    "in_and_terms": (C(1), IN(*SIZES), C(4), I(45), "ne", "and",
                     C(3), I(-500), I(900), "between", "not", "and"),
}
PROJECTIONS = [
    (C(1), C(0), I(0), "gt", C(3), "select"),                 # int lane
    (C(0), C(5), C(6), "select"),                             # mixed: double lane
    (C(6), I(1), "coalesce", I(2), "div"),                    # NULL DOUBLE cell / 2 = 0.5
    (C(0), C(1), "coalesce", I(2), "div"),
    (C(6), "is_null"),
    (C(1), IN(*SIZES)),
    (C(6), IN(-3, 0, 25, 50)),
    (NULL(0), C(0), I(0), "gt", C(0), "select"),              # CASE without ELSE
    (C(1), C(1), C(4), "eq", NULL(0), "select"),              # NULLIF
    case_chain(5),
    (NULL(1), C(3), "coalesce", I(7), "div"),
]


@pytest.fixture(scope="module")
def typed(ops):
    cols = seven_page(N_TYPED, 133, True)
    return cols, rows_of(cols), make_page(ops, cols)


@pytest.mark.parametrize("name", list(FILTERS))
def test_filter_run_whole_range_list(sess, ops, typed, name):
    cols, rows, page = typed
    prog = FILTERS[name]
    r = np.random.default_rng(7)
    check_filter(sess, ops, cols, prog, None, rows, page)
    check_filter(sess, ops, cols, prog, ("range", 5, N_TYPED - 77), rows, page)
    check_filter(sess, ops, cols, prog, ("range", 3, 0), rows, page)
    check_filter(sess, ops, cols, prog, ("list", r.integers(0, N_TYPED, 700)[::-1]), rows, page)


def test_filter_paths_are_the_planned_ones():
    paths = {n: path_of2(p, KINDS) for n, p in FILTERS.items()}
    assert paths["in_term"] == "terms" and paths["in_and_terms"] == "terms"
    assert paths["in_double_column"] == "flags" and paths["in_expression"] == "flags"
    assert paths["is_null"] == "flags" and paths["select"] == "flags"


@pytest.mark.parametrize("nullable", [True, False], ids=["nulls", "nonull"])
@pytest.mark.parametrize("filt", [None, "in_and_terms", "select"])
def test_core_filter_project(sess, ops, filt, nullable):
    """k_project after each flag kernel and alone; under TG_FP_FUSED=1 (the
    child of test_variant_fused) k_fp_count / k_fp_write"""
    cols = seven_page(N_TYPED, 134, nullable)
    f = None if filt is None else FILTERS[filt]
    for part in (PROJECTIONS[:6], PROJECTIONS[6:]):      # the fused path takes 8 at most
        check_project(sess, ops, cols, f, [(p, "i64") for p in part])
        check_project(sess, ops, cols, f, [(p, "f64") for p in part])


def test_core_const_null_alone_carries_a_bitmap(sess, ops):
    """NULL-free inputs, no DIV: the NULL literal is the only NULL source"""
    cols = seven_page(N_TYPED, 135, False)
    for filt in (None, (C(1), I(-50), "ge")):
        out = check_project(sess, ops, cols, filt,
                            [((NULL(0), C(0), I(0), "gt", C(0), "select"), "i64"),
                             ((NULL(1),), "f64"), ((NULL(0),), "i64")])
        n = len(out[0]["values"])
        assert out[0]["valid"] is not None and not unpack_bits(out[0]["valid"], n).all()
        assert unpack_bits(out[0]["valid"], n).any()
        assert not unpack_bits(out[1]["valid"], n).any()
        assert not unpack_bits(out[2]["valid"], n).any()


def test_filter_project_df(sess, ops):
    members = [10, 11, 13, 40, -75, -76, 0]
    cols = seven_page(N_TYPED, 136, True)
    bridge = df_bridge(sess, ops, members)
    try:
        for name in (None, "in_and_terms", "coalesce_lane", "is_null"):
            check_project(
                sess, ops, cols, None if name is None else FILTERS[name],
                [(PROJECTIONS[0], "i64"), (PROJECTIONS[2], "f64"), (PROJECTIONS[5], "i64")],
                make_op=lambda f, pe, ot: ops.filter_project_df(sess, f, pe, ot, bridge, 0),
                keep=lambda row: row[0] is not None and row[0] in members)
    finally:
        bridge.close()


# --------------------------------------------------------------------------
# dictionary blocks
# --------------------------------------------------------------------------
DICT_PROGS = ((C(0), IN(1, 2, -3, 77)), (C(0), IN(1, 2, -3, 77), "not"),
              (C(0), "is_null"), (C(0), I(0), "coalesce", I(1), "ge"),
              (I(0), C(0), I(0), "gt", C(0), "select", I(2), "ge"),
              (C(0), IN(1), NULL(0), "or", "is_null"))


@pytest.mark.parametrize("nulls", ["none", "outer", "dictionary", "both"])
@pytest.mark.parametrize("kind", ["i64", "i16", "bool", "f64"])
def test_dictionary_blocks(sess, ops, kind, nulls):
    """without bitmaps the verdict is computed once per entry; with one on
    either level the block is decoded first. Both equal the flat column."""
    dv, ids, dvalid, ovalid, flat = dict_case(
        kind, 9, N_TYPED, 3, nulls in ("outer", "both"), nulls in ("dictionary", "both"))
    rows = rows_of([flat])
    page = dict_page(ops, kind, dv, ids, dvalid, ovalid)
    flat_page = make_page(ops, [flat])
    for prog in DICT_PROGS:
        exp = [i for i, row in enumerate(rows) if ref_keep2(prog, row, (kind,))]
        assert ops.filter_run(sess, ops.expr(*prog), page).tolist() == exp, prog
        assert ops.filter_run(sess, ops.expr(*prog), flat_page).tolist() == exp, prog


# --------------------------------------------------------------------------
# the lookup join's residual filter
# --------------------------------------------------------------------------
B = jfm.B          # build channel b of rich_tables
JOIN_FILTERS = {
    "in_build": (B(1), IN(-2, 0, 3, jfm.POISON_I)),
    "in_build_narrow": (B(4), IN(-3000, 1000, 2000), "not"),
    "select_build": (C(1), B(1), "is_null", B(2), "select", I(2), "ge"),
    "is_null_build": (B(3), "is_null", C(1), B(1), "eq", "or"),
    "coalesce_pair": (C(4), B(3), "coalesce", I(1), "coalesce", I(2), "div", F(0.5), "ge"),
}


@pytest.mark.parametrize("join_type", [0, 1], ids=["inner", "left"])
@pytest.mark.parametrize("name", list(JOIN_FILTERS))
def test_join_filter(sess, ops, name, join_type):
    build, probe = jfm.rich_tables()
    prog = JOIN_FILTERS[name]
    kinds = tuple(c.kind for c in probe) + tuple(c.kind for c in build)
    brows, prows = jfm.cells(build), jfm.cells(probe)

    def pred(op, ob):
        vals = [ref_eval2(prog, prows[i] + brows[r], kinds) for i, r in zip(op, ob)]
        return (np.array([not v[2] and v[0] != 0 for v in vals], bool),
                np.array([v[2] for v in vals], bool))

    jfm.filtered_case(sess, ops, [build], [0], jfm.RICH_BOUT, [[probe]], [0], jfm.RICH_POUT,
                      join_type, [prog], preds=[pred], cover=False)


# --------------------------------------------------------------------------
# IN forms
# --------------------------------------------------------------------------
SPARSE = [int(v) for v in np.random.default_rng(5).choice(2 ** 40, IN_LIST_MAX, replace=False)
          - 2 ** 39]
IN_LISTS = {
    "k1": ([5], FORM_MASK),
    "k2": ([-40, 23], FORM_MASK),                                # span 64
    "k8_q16": (list(SIZES), FORM_MASK),
    "span65": ([-40, 24, 0], FORM_BITMAP),
    "bitmap_bits": ([-2000, -2000 + IN_BITMAP_BITS - 1, 7, 64, 65], FORM_BITMAP),
    "bitmap_bits_plus1": ([-2000, -2000 + IN_BITMAP_BITS, 7, 64, 65], FORM_SEARCH),
    "sparse_4096": (SPARSE, FORM_SEARCH),
    "int64_ends": ([I64_MIN, I64_MAX, 0, -1], FORM_SEARCH),
    "int64_min_side": ([I64_MIN, I64_MIN + 63], FORM_MASK),
    "int64_max_side": ([I64_MAX - 64, I64_MAX], FORM_BITMAP),
    "duplicates": ([3, 3, -7, 3, -7, 100, 100], FORM_BITMAP),
    "unsorted": ([90, -90, 5, 1000, -1000, 0], FORM_BITMAP),
    "poison": ([POISON["i64"], 17], FORM_MASK),
}


def in_column(kind, items, n, seed):
    """values drawn from the list, their neighbours and the column's ends;
    NULLs over the poison value"""
    r = np.random.default_rng(seed)
    info = None if kind == "f64" else np.iinfo(_NP[kind])
    pool = []
    for v in list(items)[:64] + [0, 1, -1]:
        pool += [v - 1, v, v + 1]
    if info is not None:
        pool = [v for v in pool if info.min <= v <= info.max] + [info.min, info.max]
    pool = [v for v in pool if I64_MIN <= v <= I64_MAX]
    vals = np.array(pool, _NP[kind])[r.integers(0, len(pool), n)]
    null = r.random(n) < 0.1
    vals[null] = POISON[kind]
    return Col(kind, vals, ~null)


@pytest.mark.parametrize("name", list(IN_LISTS))
def test_in_forms(sess, ops, name):
    items, form = IN_LISTS[name]
    assert in_form(items) == form
    cols = [in_column("i64", items, N_TYPED, 11), in_column("i32", SIZES, N_TYPED, 12)]
    rows, page = rows_of(cols), make_page(ops, cols)
    check_filter(sess, ops, cols, (C(0), IN(*items)), None, rows, page, "terms")
    check_filter(sess, ops, cols, (C(0), IN(*items), C(1), I(45), "ne", "and"),
                 None, rows, page, "terms")
    check_filter(sess, ops, cols, (C(0), IN(*items), "not"), None, rows, page, "flags")
    check_filter(sess, ops, cols, (C(0), I(0), "add", IN(*items)), None, rows, page, "flags")


@pytest.mark.parametrize("kind", ["i64", "i32", "date", "i16", "i8", "bool", "f64"])
def test_in_every_column_type(sess, ops, kind):
    """every integer width reads its own width in the set term; a DOUBLE
    column takes the interpreter and compares d == (double)item"""
    lists = ([1], [0, 1], list(SIZES), [-100, 27], [-128, 127, 5], [3, 3000, -3000],
             [2 ** 53, 2 ** 53 + 1, -1, 0])
    cols = [in_column(kind, [v for lst in lists for v in lst], N_TYPED, 13)]
    if kind == "f64":
        cols[0].values[::17] = np.nan
        cols[0].values[1::17] = -0.0
        cols[0].values[2::17] = 2.0 ** 53
    rows, page = rows_of(cols), make_page(ops, cols)
    path = "flags" if kind == "f64" else "terms"
    for items in lists:
        check_filter(sess, ops, cols, (C(0), IN(*items)), None, rows, page, path)
        check_filter(sess, ops, cols, (C(0), IN(*items), C(0), I(2), "ne", "and"),
                     None, rows, page, path)


def test_in_terms_at_fterm_max(sess, ops, typed):
    """two set terms and compares: FTERM_MAX terms take k_filter_terms, one
    more takes the interpreter; same answer"""
    cols, rows, page = typed
    wide = [(C(j % 5), I(-95 + j), "ge") for j in range(FTERM_MAX)]
    two = [(C(1), IN(*range(-100, 101, 3))), (C(3), IN(*range(-3000, 3001, 5)))]
    at_max = chain(*(two + wide[:FTERM_MAX - 2]))
    over = chain(*(two + wide[:FTERM_MAX - 1]))
    check_filter(sess, ops, cols, at_max, None, rows, page, "terms")
    check_filter(sess, ops, cols, over, None, rows, page, "flags")
    kept = ops.filter_run(sess, ops.expr(*at_max), page)
    assert 0 < len(kept) < N_TYPED


def test_in_list_max_plus_one_is_rejected(sess, ops, typed):
    cols, rows, page = typed
    ok = ops.expr(C(1), IN(*range(IN_LIST_MAX)))
    assert len(ops.filter_run(sess, ok, page)) > 0
    big = ops.expr(C(1), IN(*range(IN_LIST_MAX + 1)))
    expect_error(lambda: ops.filter_run(sess, big, page), TG_ERR_UNSUPPORTED, "IN list")
    expect_error(lambda: ops.filter_project(sess, big, [ops.expr(C(0))]),
                 TG_ERR_UNSUPPORTED, "IN list")
    expect_error(lambda: ops.filter_project(sess, None, [big]), TG_ERR_UNSUPPORTED, "IN list")


def test_rejects_varchar_under_is_null(sess, ops):
    cols = [Col("i64", np.arange(30)), Col("str", [b"ab", b"", b"c"] * 10)]
    page = make_page(ops, cols)
    for prog in ((C(1), "is_null"), (C(1), IN(1, 2)), (C(0), C(1), "coalesce", I(0), "ge")):
        expect_error(lambda: ops.filter_run(sess, ops.expr(*prog), page),
                     TG_ERR_UNSUPPORTED, "VARCHAR")


# --------------------------------------------------------------------------
# row counts
# --------------------------------------------------------------------------
ROW_COUNTS = (0, 1, 63, 64, 65, CHUNK - 1, CHUNK + 1)


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts(sess, ops, n):
    """an IN term of each form and a SELECT projection at the wave and chunk
    edges; the reference is vectorised here (numpy isin / where)"""
    r = np.random.default_rng(n + 1)
    null = r.random(n) < 0.1
    a = np.where(null, POISON["i32"], r.integers(-100, 4200, n)).astype(np.int32)
    b = r.integers(-50, 50, n).astype(np.int64)
    cols = [Col("i32", a, ~null), Col("i64", b)]
    page = make_page(ops, cols)
    for items in (list(SIZES), list(range(0, IN_BITMAP_BITS, 3)), list(range(0, 50000, 13))):
        got = ops.filter_run(sess, ops.expr(C(0), IN(*items)), page)
        exp = np.flatnonzero(~null & np.isin(a, items)).astype(np.int32)
        assert np.array_equal(got, exp), (n, len(items))
    op = ops.filter_project(sess, None, [ops.expr(C(1), C(0), IN(*SIZES), C(0), "select")],
                            [ops.TG_BIGINT])
    try:
        op.add_input(page)
        out = op.drain()[0][0]
    finally:
        op.close()
    take = ~null & np.isin(a, SIZES)
    assert np.array_equal(out["values"], np.where(take, a, b))
    assert out["valid"] is None or unpack_bits(out["valid"], n).all()


def test_grid_stride_in_term_and_select_projection(sess, ops):
    """n = one grid of threads + 257: the grid-stride loops take a second trip"""
    assert GRID_N > GRID_THREADS
    base, cols = grid_cols()               # INTEGER, DOUBLE; periodic in PERIOD rows
    kinds = kinds_of(base)
    page = make_page(ops, cols)
    prog = (C(0), IN(1, 2, 5, -3), C(1), F(1.0), "le", "and")
    assert path_of2(prog, kinds) == "terms"
    keep = tiled([ref_keep2(prog, row, kinds) for row in rows_of(base)])
    got = ops.filter_run(sess, ops.expr(*prog), page)
    assert np.array_equal(got, np.flatnonzero(keep).astype(np.int32))
    proj = (C(1), C(0), IN(1, 2, 5, -3), C(0), "select")
    vals = [ref_eval2(proj, row, kinds) for row in rows_of(base)]
    assert not any(v[2] for v in vals) and not any(v[1] for v in vals)
    op = ops.filter_project(sess, None, [ops.expr(*proj)], [ops.TG_DOUBLE])
    try:
        op.add_input(page)
        out = op.drain()[0][0]
    finally:
        op.close()
    exp = tiled(np.array([v[0] for v in vals], np.float64))
    assert np.array_equal(out["values"].view(np.int64), exp.view(np.int64))


# --------------------------------------------------------------------------
# the seeded random programs of the reference file
# --------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(4))
def test_random_programs(sess, ops, block):
    """all three flag kernels: test_expr_reference.py asserts that the programs
    reach each of them"""
    cols, _ = random_rows()
    page = make_page(ops, cols)
    for k in range(block, N_PROGRAMS, 4):
        prog, exp = random_case(k)
        got = ops.filter_run(sess, ops.expr(*prog), page)
        assert got.tolist() == exp, (k, path_of2(prog, KINDS), prog)


# --------------------------------------------------------------------------
# fused variant: the test_core_* subset in a fresh child under TG_FP_FUSED=1
# (the variable is read once per process)
# --------------------------------------------------------------------------
def test_variant_fused():
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x",
           "-k", "test_core", "-p", "no:cacheprovider"]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, TG_FP_FUSED="1"), cwd=_ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
    except subprocess.TimeoutExpired:
        pytest.exit("expr matrix child (TG_FP_FUSED=1) hit its time limit: "
                    "nothing more is started on the GPU", returncode=3)
    if r.returncode < 0 or r.returncode >= 128:
        pytest.exit("expr matrix child (TG_FP_FUSED=1) ended on a signal "
                    f"(status {r.returncode}): nothing more is started on the "
                    f"GPU\n{r.stdout[-3000:]}", returncode=3)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:]
