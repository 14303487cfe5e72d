"""Filter / projection parity matrix: tg_filter_run, FilterProjectOp, the
dynamic filter and the dictionary-aware filter of trino_amd/csrc/
ops_filter.hip (with the page decode of ops_core.hip) against an exact
reference written here in plain Python (no trino_amd, no torch, no oracle).

Reference: ref_eval(prog, row) is a postfix interpreter over Python ints,
floats and None that returns (value, is_int, is_null):
  - integer lanes are Python ints. Every input of this file keeps every
    intermediate inside int64 (tests/test_oracle_units.py asserts it for the
    random programs): integer overflow and INT64_MIN / -1 are OUT OF SCOPE,
    because Trino raises there and the C ABI has no per-row error channel;
  - a mixed int/double operation coerces the int side with float(i);
  - integer division truncates toward zero and `/ 0` gives NULL; double
    division is IEEE (x/0 = +-inf, 0/0 = NaN);
  - AND, OR, NOT are Kleene three-valued logic; BETWEEN is Kleene
    `a >= lo AND a <= hi`;
  - compares are exact in int64 when both sides are ints, else IEEE on
    doubles: NaN compares false except under `!=`;
  - a filter keeps a row iff the result is non-NULL and truthy (!= 0).

Comparison: selection vectors bit-exact and in order. Projections bit-exact
too: the library is built with -ffp-contract=off and every instruction is
one IEEE double operation, so the same operation per instruction in Python's
float64 agrees to the last bit; no tolerance anywhere. The one equivalence:
IEEE 754 leaves sign and payload of a NaN *produced* by an operation to the
implementation, so a NaN result is compared as "is NaN" (NaNs that are merely
copied by an identity projection are compared by their bits). Where the
reference says NULL only the validity bit is compared.

Every NULL input cell carries a poison value in its data word that would
change the verdict if it were read.

Not reached: the second recursion level of run_scan_i32 (needs more than
2*FSCAN_CHUNK^2 = 8M scanned entries) and integer overflow (above).

Host-side checks of this reference and of the shapes are in
tests/test_oracle_units.py::TestFilterMatrixHost (no GPU).
"""
import functools
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "trino_amd", "csrc")

TG_ERR_INVALID_ARG, TG_ERR_UNSUPPORTED = 1, 6


# --------------------------------------------------------------------------
# constants of the code under test, parsed from its sources
# --------------------------------------------------------------------------
@functools.lru_cache(None)
def source_constants():
    flt = open(os.path.join(_CSRC, "ops_filter.hip")).read()
    common = open(os.path.join(_CSRC, "common.h")).read()

    def one(pat, text):
        m = re.search(pat, text)
        assert m, pat
        return int(m.group(1))

    return dict(
        CHUNK=one(r"#define CHUNK (\d+)", flt),
        FSCAN_CHUNK=one(r"#define FSCAN_CHUNK (\d+)", flt),
        FTERM_MAX=one(r"#define FTERM_MAX (\d+)", flt),
        MAX_STACK=one(r"#define MAX_STACK (\d+)", flt),
        SCAN_SMALL_FACTOR=one(r"if \(n <= (\d+) \* FSCAN_CHUNK\)", flt),
        TG_BLOCK=one(r"constexpr int TG_BLOCK = (\d+);", common),
        TG_MAX_BLOCKS=one(r"constexpr int TG_MAX_BLOCKS = (\d+);", common),
    )


# the values the shapes below assume; TestFilterMatrixHost pins them to the
# parsed ones, so a changed constant fails loudly instead of silently
# moving a shape off its edge
CHUNK = 16384
FSCAN_CHUNK = 2048
FTERM_MAX = 8
MAX_STACK = 6
GRID_THREADS = 256 * 2048
GRID_N = GRID_THREADS + 257

EDGE_SIZES = (0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7)


def edge_sizes():
    """the compaction sizes; every n >= 63 also as n + 3, which is never a
    multiple of 8 here, so the byte tail of k_count_chunk runs at each edge"""
    out = list(EDGE_SIZES) + [n + 3 for n in EDGE_SIZES if n >= 63]
    assert all((n + 3) % 8 for n in EDGE_SIZES if n >= 63)
    return sorted(out)


VARCHAR_COUNTS = (0, 1, 2 * FSCAN_CHUNK, 2 * FSCAN_CHUNK + 1, 3 * FSCAN_CHUNK + 1)
N_TYPED = 1031
KINDS = ("i64", "i32", "date", "i16", "i8", "bool", "f64")
_NP = {"i64": np.int64, "i32": np.int32, "date": np.int32, "i16": np.int16,
       "i8": np.int8, "bool": np.int8, "f64": np.float64}
CMPS = ("le", "lt", "ge", "gt", "eq", "ne")


# --------------------------------------------------------------------------
# reference
# --------------------------------------------------------------------------
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


class LeftInt64(Exception):
    """an integer lane of the reference left int64 (out of scope)"""


def _fdiv(a, b):
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _truthy(v):
    return v[0] != 0


def _cmp(op, a, b):
    """typed compare of two non-NULL stack values"""
    if a[1] and b[1]:
        x, y = a[0], b[0]
    else:
        x, y = float(a[0]), float(b[0])     # never Python's exact int-vs-float
    return {"le": x <= y, "lt": x < y, "ge": x >= y, "gt": x > y,
            "eq": x == y, "ne": x != y}[op]


def _kleene_and(a, b):
    """a, b: True / False / None"""
    if a is False or b is False:
        return False
    if a is None or b is None:
        return None
    return True


def _tv(v):
    return None if v[2] else _truthy(v)


def _bool(t):
    return (0, True, True) if t is None else (1 if t else 0, True, False)


def ref_eval(prog, row):
    """prog: postfix items ('col', i) ('i64', v) ('f64', v) or an op name;
    row: sequence of int / float / None. Returns (value, is_int, is_null)."""
    st = []
    for it in prog:
        if isinstance(it, tuple):
            kind, v = it
            if kind == "col":
                x = row[v]
                st.append((0, True, True) if x is None
                          else (x, isinstance(x, int), False))
            elif kind == "i64":
                st.append((int(v), True, False))
            else:
                st.append((float(v), False, False))
        elif it in ("add", "sub", "mul", "div"):
            b = st.pop()
            a = st.pop()
            isint = a[1] and b[1]
            if a[2] or b[2]:
                st.append((0, isint, True))
            elif isint:
                if it == "div":
                    if b[0] == 0:
                        st.append((0, True, True))
                        continue
                    q = abs(a[0]) // abs(b[0])
                    r = q if (a[0] < 0) == (b[0] < 0) else -q
                else:
                    r = {"add": a[0] + b[0], "sub": a[0] - b[0], "mul": a[0] * b[0]}[it]
                if not I64_MIN <= r <= I64_MAX:
                    raise LeftInt64(it)
                st.append((r, True, False))
            else:
                x, y = float(a[0]), float(b[0])
                r = {"add": lambda: x + y, "sub": lambda: x - y,
                     "mul": lambda: x * y, "div": lambda: _fdiv(x, y)}[it]()
                st.append((r, False, False))
        elif it in CMPS:
            b = st.pop()
            a = st.pop()
            st.append(_bool(None if (a[2] or b[2]) else _cmp(it, a, b)))
        elif it == "and":
            b = st.pop()
            a = st.pop()
            st.append(_bool(_kleene_and(_tv(a), _tv(b))))
        elif it == "or":
            b = st.pop()
            a = st.pop()
            na, nb = _tv(a), _tv(b)
            r = _kleene_and(None if na is None else not na, None if nb is None else not nb)
            st.append(_bool(None if r is None else not r))
        elif it == "not":
            a = _tv(st.pop())
            st.append(_bool(None if a is None else not a))
        elif it == "between":
            c = st.pop()
            b = st.pop()
            a = st.pop()
            ge = None if (a[2] or b[2]) else _cmp("ge", a, b)
            le = None if (a[2] or c[2]) else _cmp("le", a, c)
            st.append(_bool(_kleene_and(ge, le)))
        else:
            raise ValueError(it)
    assert len(st) == 1, "malformed program"
    return st[0]


def ref_keep(prog, row):
    v = ref_eval(prog, row)
    return (not v[2]) and _truthy(v)


def stack_profile(prog):
    """(max depth, final depth, underflowed) of a postfix program"""
    sp = mx = 0
    under = False
    for it in prog:
        if isinstance(it, tuple):
            sp += 1
        elif it == "not":
            pass
        elif it == "between":
            sp -= 2
        else:
            sp -= 1
        mx = max(mx, sp)
        under |= sp < 1
    return mx, sp, under


def _is_const(it):
    return isinstance(it, tuple) and it[0] in ("i64", "f64")


def _is_col(it):
    return isinstance(it, tuple) and it[0] == "col"


def _match_term(p, i):
    """length of the conjunction-path term at p[i:], 0 if none (the grammar
    of parse_fterms: IN-pair over ONE column, BETWEEN, col-const, col-col)"""
    if i >= len(p) or not _is_col(p[i]):
        return 0
    if (i + 6 < len(p) and _is_const(p[i + 1]) and p[i + 2] == "eq" and
            p[i + 3] == p[i] and _is_const(p[i + 4]) and p[i + 5] == "eq" and
            p[i + 6] == "or"):
        return 7
    if i + 3 < len(p) and _is_const(p[i + 1]) and _is_const(p[i + 2]) and p[i + 3] == "between":
        return 4
    if i + 2 < len(p) and (_is_const(p[i + 1]) or _is_col(p[i + 1])) and p[i + 2] in CMPS:
        return 3
    return 0


def count_terms(prog):
    """number of terms if prog is T (T AND)*, else 0"""
    p = list(prog)
    k = _match_term(p, 0)
    if not k:
        return 0
    i, nt = k, 1
    while i < len(p):
        k = _match_term(p, i)
        if not k or i + k >= len(p) or p[i + k] != "and":
            return 0
        i += k + 1
        nt += 1
    return nt


def path_of(prog):
    """the flag kernel run_filter picks: 'cmp', 'terms' or 'flags'"""
    p = list(prog)
    if len(p) == 3 and _is_col(p[0]) and _is_const(p[1]) and p[2] in CMPS:
        return "cmp"
    nt = count_terms(p)
    return "terms" if 0 < nt <= FTERM_MAX else "flags"


# --------------------------------------------------------------------------
# columns and pages
# --------------------------------------------------------------------------
POISON = {"i64": 1, "i32": 1, "date": 1, "i16": 1, "i8": 1, "bool": 1, "f64": 1.0}


class Col:
    """kind, numpy values and valid (bool array, None = no bitmap); 'str'
    columns hold a list of bytes"""

    def __init__(self, kind, values, valid=None):
        self.kind = kind
        self.values = (list(values) if kind == "str"
                       else np.ascontiguousarray(values, _NP[kind]))
        self.valid = None if valid is None else np.asarray(valid, bool)

    def __len__(self):
        return len(self.values)

    def cells(self):
        if self.kind == "str":
            vals = list(self.values)
        else:
            vals = self.values.tolist()      # Python ints / floats
        if self.valid is not None:
            vals = [v if ok else None for v, ok in zip(vals, self.valid.tolist())]
        return vals


def rows_of(cols):
    return list(zip(*[c.cells() for c in cols]))


def pack_bits(valid):
    n = len(valid)
    b = np.zeros(max((n + 63) // 64, 1) * 64, bool)
    b[:n] = valid
    return np.packbits(b, bitorder="little").view(np.uint64).copy()


def unpack_bits(words, n):
    if words is None:
        return np.ones(n, bool)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def tg_type(ops, kind):
    return {"i64": ops.TG_BIGINT, "i32": ops.TG_INTEGER, "date": ops.TG_DATE,
            "i16": ops.TG_SMALLINT, "i8": ops.TG_TINYINT, "bool": ops.TG_BOOLEAN,
            "f64": ops.TG_DOUBLE, "str": ops.TG_VARCHAR}[kind]


def make_page(ops, cols):
    columns, valids = [], []
    for c in cols:
        if c.kind == "str":
            lens = np.array([len(v) for v in c.values], np.int64)
            offs = np.zeros(len(lens) + 1, np.int32)
            offs[1:] = np.cumsum(lens)
            data = np.frombuffer(b"".join(c.values) + b"\0", np.uint8).copy()
            columns.append((data, offs))
        else:
            columns.append(c.values)
        valids.append(None if c.valid is None else pack_bits(c.valid))
    if any(c.kind == "str" for c in cols):
        page = ops.page_with_varchar(columns, valids=valids)
    else:
        page = ops.page_from_numpy(columns, valids=valids)
    for i, c in enumerate(cols):
        page.blocks[i].type = tg_type(ops, c.kind)
    return page


_INT_POOL = (-3, -2, -1, 0, 0, 1, 1, 2, 3, 5)
_F64_POOL = (-2.5, -1.0, -0.0, 0.0, 0.5, 1.0, 1.0, 1.5, 2.0, 3.25)
F64_SPECIALS = (-0.0, 0.0, math.inf, -math.inf, math.nan, 1.0, -1.0, 0.5)


def typed_col(kind, n, seed, nullable, pool=None):
    """n values of `kind` drawn from a small pool around the constants the
    programs use (so every operator both passes and fails), about 10 %
    NULLs over a poison value when `nullable`"""
    r = np.random.default_rng(seed)
    if pool is None:
        pool = (_F64_POOL if kind == "f64" else (0, 1, 1, 0, 1) if kind == "bool"
                else _INT_POOL)
    vals = np.array(pool, _NP[kind])[r.integers(0, len(pool), n)]
    if not nullable:
        return Col(kind, vals)
    null = r.random(n) < 0.1
    vals[null] = POISON[kind]
    return Col(kind, vals, ~null)


def seven_page(n, seed, nullable=True):
    """one column of every fixed-width type, |value| < 2^31 in every cell"""
    r = np.random.default_rng(seed)
    cols = []
    for j, kind in enumerate(KINDS):
        if kind == "f64":
            vals = np.round(r.uniform(-100, 100, n) * 4) / 4
        elif kind == "bool":
            vals = r.integers(0, 2, n)
        elif kind == "i8":
            vals = r.integers(-100, 101, n)
        elif kind == "i16":
            vals = r.integers(-3000, 3001, n)
        else:
            vals = r.integers(-100, 101, n)
        vals = np.asarray(vals, _NP[kind])
        if nullable:
            null = r.random(n) < 0.08
            vals[null] = POISON[kind]
            cols.append(Col(kind, vals, ~null))
        else:
            cols.append(Col(kind, vals))
    return cols


# --------------------------------------------------------------------------
# runners
# --------------------------------------------------------------------------
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


def selection(ops, kind, a, b=None):
    """('range', offset, size) or ('list', positions)"""
    sel = ops.TgSelected()
    if kind == "range":
        sel.is_list, sel.offset, sel.size = 0, a, b
        return sel, list(range(a, a + b))
    pos = np.ascontiguousarray(a, np.int32)
    sel.is_list, sel.offset, sel.size = 1, 0, len(pos)
    sel.positions = pos.ctypes.data
    sel._keep = pos
    return sel, pos.tolist()


def _row_key(row):
    """dict key that tells -0.0 from 0.0 (they hash and compare alike)"""
    return row, tuple(math.copysign(1.0, x) for x in row if x.__class__ is float)


def ref_filter(prog, rows, positions=None):
    """positions kept, in order; the verdict of equal rows is computed once"""
    if positions is None:
        positions = range(len(rows))
    seen, out = {}, []
    for i in positions:
        k = _row_key(rows[i])
        v = seen.get(k)
        if v is None:
            v = seen[k] = ref_keep(prog, rows[i])
        if v:
            out.append(i)
    return out


def check_filter(sess, ops, cols, prog, sel=None, rows=None, page=None, path=None):
    if path is not None:
        assert path_of(prog) == path, (path_of(prog), prog)
    rows = rows_of(cols) if rows is None else rows
    page = make_page(ops, cols) if page is None else page
    tsel, positions = (None, None) if sel is None else selection(ops, *sel)
    got = ops.filter_run(sess, ops.expr(*prog), page, tsel)
    exp = ref_filter(prog, rows, positions)
    assert len(got) == len(exp), (len(got), len(exp), prog)
    bad = np.flatnonzero(got != np.array(exp, np.int32))
    assert len(bad) == 0, f"{prog}: first difference at output {bad[0]}"


def ref_project(prog, out_kind, rows, positions):
    """expected (values list, valid list) of one projection"""
    vals, valid = [], []
    for i in positions:
        v = ref_eval(prog, rows[i])
        valid.append(not v[2])
        if v[2]:
            vals.append(0)
        elif out_kind == "i64":
            vals.append(v[0] if v[1] else int(v[0]))
        else:
            vals.append(float(v[0]))
    return vals, valid


def assert_projection(got, exp_vals, exp_valid, kind, what):
    n = len(exp_vals)
    assert len(got["values"]) == n, (what, len(got["values"]), n)
    gv = unpack_bits(got["valid"], n)
    assert np.array_equal(gv, np.array(exp_valid, bool)), f"{what}: validity"
    ok = np.array(exp_valid, bool)
    if kind == "str":
        bad = [k for k in range(n) if ok[k] and got["values"][k] != exp_vals[k]]
        assert not bad, f"{what}: bytes differ first at {bad[0]}"
        assert not any(len(got["values"][k]) for k in range(n) if not ok[k]), \
            f"{what}: a NULL VARCHAR cell has bytes"
        return
    g = np.asarray(got["values"])
    e = np.array(exp_vals, _NP[kind]) if n else np.empty(0, _NP[kind])
    assert g.dtype == e.dtype, (what, g.dtype, e.dtype)
    if kind == "f64":
        both_nan = np.isnan(g) & np.isnan(e)
        differ = (g.view(np.int64) != e.view(np.int64)) & ~both_nan
    else:
        differ = g != e
    bad = np.flatnonzero(differ & ok)
    assert len(bad) == 0, f"{what}: row {bad[0]} got {g[bad[0]]!r} expected {e[bad[0]]!r}"


def check_project(sess, ops, pages, filt, projs, make_op=None, keep=None):
    """pages: list of column lists fed to ONE operator. projs: list of
    (prog, out_kind); an identity program takes its source column's kind.
    keep(row) is an extra reference-side row test (the dynamic filter)."""
    out_types = [tg_type(ops, k if k != "str" else "f64") for _, k in projs]
    f = ops.expr(*filt) if filt is not None else None
    pe = [ops.expr(*p) for p, _ in projs]
    op = (make_op(f, pe, out_types) if make_op
          else ops.filter_project(sess, f, pe, out_types))
    try:
        outs = []
        for cols in pages:
            op.add_input(make_page(ops, cols))
        outs = op.drain()
    finally:
        op.close()
    assert len(outs) == len(pages)
    for cols, out in zip(pages, outs):
        rows = rows_of(cols)
        positions = [i for i in range(len(rows))
                     if (filt is None or ref_keep(filt, rows[i])) and
                     (keep is None or keep(rows[i]))]
        assert len(out) == len(projs)
        for j, (prog, kind) in enumerate(projs):
            if len(prog) == 1 and _is_col(prog[0]):       # identity: bits travel
                src = cols[prog[0][1]]
                cells = src.cells()
                ev = [cells[i] for i in positions]
                exp_valid = [v is not None for v in ev]
                assert out[j]["type"] == tg_type(ops, src.kind), (prog, out[j]["type"])
                if src.kind == "str":
                    assert_projection(out[j], ev, exp_valid, "str", prog)
                else:
                    g = np.asarray(out[j]["values"])
                    e = src.values[np.array(positions, np.int64)]
                    assert len(g) == len(e), (prog, len(g), len(e))
                    gvalid = unpack_bits(out[j]["valid"], len(e))
                    assert np.array_equal(gvalid, np.array(exp_valid, bool)), (prog, "validity")
                    view = np.int64 if src.kind == "f64" else _NP[src.kind]
                    bad = np.flatnonzero((g.view(view) != e.view(view)) & gvalid)
                    assert len(bad) == 0, f"{prog}: identity differs at {bad[0]}"
                continue
            ev, exp_valid = ref_project(prog, kind, rows, positions)
            assert out[j]["type"] == tg_type(ops, kind), (prog, out[j]["type"])
            assert_projection(out[j], ev, exp_valid, kind, prog)


def expect_error(fn, status, *words):
    import trino_amd
    with pytest.raises(trino_amd.TrinoGpuError) as ei:
        fn()
    msg = str(ei.value)
    assert msg.startswith(f"status {status}:"), msg
    for w in words:
        assert w in msg, msg


C = lambda i: ("col", i)           # noqa: E731
I = lambda v: ("i64", v)           # noqa: E731
F = lambda v: ("f64", v)           # noqa: E731


# --------------------------------------------------------------------------
# compaction edges: k_count_chunk, run_scan_i32 (one launch), k_compact
# --------------------------------------------------------------------------
def pattern_flags(name, n):
    i = np.arange(n)
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    if name == "alternating":
        return i % 2 == 0
    if name == "lane63":
        return i % 64 == 63
    if name == "chunk_last":
        return (i % CHUNK == CHUNK - 1) | (i == n - 1)
    if name == "first_chunk_only":
        return i < CHUNK
    if name == "second_chunk_only":
        return (i >= CHUNK) & (i < 2 * CHUNK)
    raise ValueError(name)


PATTERNS = ("all", "none", "alternating", "lane63", "chunk_last",
            "first_chunk_only", "second_chunk_only")
# one predicate per flag kernel, each true exactly where column 0 is 1
EDGE_PROGS = ((C(0), I(1), "eq"),
              (C(0), I(1), "eq", C(0), I(0), "gt", "and"),
              (C(0), I(1), "eq", "not", "not"))


def edge_cols(name, n):
    flags = pattern_flags(name, n)
    return [Col("i32", flags.astype(np.int32))], flags


@pytest.mark.parametrize("name", PATTERNS)
def test_compaction_edges(sess, ops, name):
    """k_count_chunk word loop and byte tail, k_scan_serial, k_compact over
    every size edge x pass pattern; the flag kernel rotates with the size"""
    for k, n in enumerate(edge_sizes()):
        cols, flags = edge_cols(name, n)
        prog = EDGE_PROGS[k % 3]
        got = ops.filter_run(sess, ops.expr(*prog), make_page(ops, cols))
        exp = np.flatnonzero(flags).astype(np.int32)
        assert ref_filter(prog, rows_of(cols)) == exp.tolist()   # reference agrees
        assert np.array_equal(got, exp), (name, n, path_of(prog))


def test_core_compaction_fused(sess, ops):
    """the same sizes and patterns through FilterProjectOp (k_fp_count /
    k_fp_write under TG_FP_FUSED=1, k_filter_* + k_gather otherwise)"""
    for k, n in enumerate(edge_sizes()):
        name = PATTERNS[k % len(PATTERNS)]
        flags = pattern_flags(name, n)
        r = np.random.default_rng(n)
        null = r.random(n) < 0.2
        cols = [Col("i32", flags.astype(np.int32)),
                Col("i64", np.where(null, 7, np.arange(n)), ~null)]
        check_project(sess, ops, [cols], EDGE_PROGS[k % 3],
                      [((C(1),), "i64"), ((C(1), I(3), "mul", C(0), "add"), "i64")])


# --------------------------------------------------------------------------
# selections
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sel_page(ops):
    n = CHUNK + 100
    cols = [typed_col("i64", n, 5, True), typed_col("f64", n, 6, True)]
    return cols, rows_of(cols), make_page(ops, cols)


@pytest.mark.parametrize("offset", [0, 5, CHUNK - 3])
def test_selection_range_with_offset(sess, ops, sel_page, offset):
    cols, rows, page = sel_page
    for size in (0, 1, 70, len(rows) - offset - 1):
        for prog in ((C(0), I(1), "ge"), (C(0), I(0), "ge", C(1), F(1.0), "le", "and"),
                     (C(0), C(1), "add", F(1.0), "gt")):
            check_filter(sess, ops, cols, prog, ("range", offset, size), rows, page)


@pytest.mark.parametrize("order", ["ascending", "descending", "repeated", "empty"])
def test_selection_list(sess, ops, sel_page, order):
    """the output echoes the list's entries in list order"""
    cols, rows, page = sel_page
    r = np.random.default_rng(3)
    pos = np.sort(r.choice(len(rows), 3000, replace=False))
    pos = {"ascending": pos, "descending": pos[::-1],
           "repeated": r.integers(0, len(rows), 3000) // 7 * 7 % len(rows),
           "empty": pos[:0]}[order]
    for prog in ((C(0), I(1), "ge"), (C(0), I(0), "ge", C(1), F(1.0), "le", "and"),
                 (C(0), C(1), "add", F(1.0), "gt")):
        check_filter(sess, ops, cols, prog, ("list", pos), rows, page)


# --------------------------------------------------------------------------
# k_filter_cmp: six operators x column type x bitmap x constant kind
# --------------------------------------------------------------------------
@pytest.mark.parametrize("nullable", [False, True], ids=["nonull", "nulls"])
@pytest.mark.parametrize("kind", KINDS)
def test_filter_cmp_types(sess, ops, kind, nullable):
    cols = [typed_col(kind, N_TYPED, 17, nullable)]
    rows, page = rows_of(cols), make_page(ops, cols)
    for op in CMPS:
        for const in (I(1), F(1.0), F(0.5), I(0)):
            check_filter(sess, ops, cols, (C(0), const, op), None, rows, page, path="cmp")


def big_cols():
    """BIGINT around 2^53 (rounds in a double lane) and 2^60 (exact lane)"""
    r = np.random.default_rng(9)
    a = 2 ** 53 + r.integers(-2, 3, N_TYPED)
    b = 2 ** 60 + r.integers(-2, 3, N_TYPED)
    null = r.random(N_TYPED) < 0.1
    return [Col("i64", a), Col("i64", np.where(null, 2 ** 60 + 1, b), ~null)]


@pytest.mark.parametrize("op", CMPS)
def test_filter_cmp_bigint_lanes(sess, ops, op):
    """2^53+1 against an F64 constant compares as doubles on both sides;
    2^60+1 against an I64 constant compares exactly"""
    cols = big_cols()
    rows, page = rows_of(cols), make_page(ops, cols)
    check_filter(sess, ops, cols, (C(0), F(float(2 ** 53)), op), None, rows, page, "cmp")
    check_filter(sess, ops, cols, (C(0), I(2 ** 53 + 1), op), None, rows, page, "cmp")
    check_filter(sess, ops, cols, (C(1), I(2 ** 60 + 1), op), None, rows, page, "cmp")
    check_filter(sess, ops, cols, (C(1), F(float(2 ** 60)), op), None, rows, page, "cmp")


@pytest.mark.parametrize("op", CMPS)
def test_filter_cmp_double_specials(sess, ops, op):
    cols = [typed_col("f64", N_TYPED, 4, True, pool=F64_SPECIALS)]
    rows, page = rows_of(cols), make_page(ops, cols)
    for const in (F(0.0), F(-0.0), F(math.inf), F(-math.inf), F(math.nan), I(0), I(1)):
        check_filter(sess, ops, cols, (C(0), const, op), None, rows, page, "cmp")


# --------------------------------------------------------------------------
# k_filter_terms
# --------------------------------------------------------------------------
def chain(*terms):
    out = list(terms[0])
    for t in terms[1:]:
        out += list(t) + ["and"]
    return tuple(out)


def in_pair(c, v1, v2):
    return (C(c), v1, "eq", C(c), v2, "eq", "or")


# columns of seven_page: 0 i64, 1 i32, 2 date, 3 i16, 4 i8, 5 bool, 6 f64
T_CONST = (C(0), I(-20), "ge")
T_CONST_F = (C(6), F(10.25), "lt")
T_COLCOL_II = (C(0), C(1), "le")
T_COLCOL_IF = (C(2), C(6), "gt")
T_COLCOL_FF = (C(6), C(6), "eq")
T_BETWEEN = (C(3), I(-2000), I(2500), "between")
T_BETWEEN_F = (C(1), F(-50.5), I(60), "between")
T_BETWEEN_EMPTY = (C(1), I(10), I(-10), "between")
T_IN = in_pair(5, I(1), I(7))
T_IN_F = in_pair(6, F(0.25), I(1))
WIDE = [(C(j % 5), I(-95 + j), "ge") for j in range(FTERM_MAX + 1)]


def terms_programs():
    """(program, expected path) for the conjunction fast path and its near
    misses"""
    t = []
    for single in (T_CONST, T_CONST_F, T_COLCOL_II, T_COLCOL_IF, T_COLCOL_FF,
                   T_BETWEEN, T_BETWEEN_F, T_BETWEEN_EMPTY, T_IN, T_IN_F):
        t.append((chain(single, (C(5), I(0), "ge")), "terms"))
        t.append((chain(single, single), "terms"))
    t.append((T_BETWEEN, "terms"))              # kinds 1..3 alone (kind 0 alone
    t.append((T_IN, "terms"))                   # is the cmp fast path)
    t.append((T_COLCOL_II, "terms"))
    t.append((chain(*WIDE[:FTERM_MAX]), "terms"))
    t.append((chain(T_IN, *WIDE[:FTERM_MAX - 1]), "terms"))
    t.append((chain(T_CONST, T_BETWEEN, T_COLCOL_IF, T_IN, T_CONST_F, T_IN_F,
                    T_BETWEEN_F, T_COLCOL_II), "terms"))
    t.append((chain(*WIDE), "flags"))           # FTERM_MAX + 1 terms
    t.append((chain(T_IN, T_CONST, T_BETWEEN), "terms"))       # IN first
    t.append((chain(T_CONST, T_IN, T_BETWEEN), "terms"))       # IN middle
    t.append((chain(T_CONST, T_BETWEEN, T_IN), "terms"))       # IN last
    # near misses of the grammar
    t.append(((C(4), I(3), "eq", C(3), I(-7), "eq", "or"), "flags"))   # two columns
    t.append((chain(T_CONST, (C(4), I(3), "eq", C(1), I(3), "eq", "or")), "flags"))
    t.append((T_CONST + T_BETWEEN + ("or",), "flags"))                  # term, term, or
    t.append((chain(T_CONST, T_BETWEEN) + ("not",), "flags"))           # trailing not
    t.append((T_BETWEEN + ("not",), "flags"))
    return t


@pytest.mark.parametrize("nullable", [False, True], ids=["nonull", "nulls"])
def test_filter_terms(sess, ops, nullable):
    cols = seven_page(N_TYPED, 21, nullable)
    rows, page = rows_of(cols), make_page(ops, cols)
    for prog, path in terms_programs():
        check_filter(sess, ops, cols, prog, None, rows, page, path)


def test_filter_terms_big_int_and_specials(sess, ops):
    """exact int64 terms above 2^53, and +-0 / inf / NaN through every term
    kind"""
    cols = big_cols() + [typed_col("f64", N_TYPED, 4, True, pool=F64_SPECIALS),
                         typed_col("f64", N_TYPED, 5, False, pool=F64_SPECIALS)]
    rows, page = rows_of(cols), make_page(ops, cols)
    for prog in (chain((C(1), I(2 ** 60 + 1), "eq"), (C(0), F(float(2 ** 53)), "eq")),
                 chain((C(1), I(2 ** 60), I(2 ** 60 + 1), "between"), (C(0), I(2 ** 53 + 1), "ne")),
                 chain(in_pair(1, I(2 ** 60 - 1), I(2 ** 60 + 2)), (C(0), C(1), "lt")),
                 chain((C(2), C(3), "eq"), (C(3), C(3), "eq")),
                 chain((C(2), C(3), "ne"), (C(2), F(-math.inf), F(0.0), "between")),
                 chain(in_pair(2, F(-0.0), F(math.inf)), (C(3), F(math.nan), "ne")),
                 (C(2), F(math.nan), F(math.nan), "between"),
                 (C(0), C(2), "ge")):
        check_filter(sess, ops, cols, prog, None, rows, page, "terms")


# --------------------------------------------------------------------------
# k_filter_flags: the interpreter
# --------------------------------------------------------------------------
def deep_program(depth):
    """pushes `depth` values before the first operator: max stack == depth"""
    p = [C(j % 5) for j in range(depth)]
    p += ["add"] * (depth - 1)
    return tuple(p) + (I(0), "gt")


def flags_programs():
    return [
        (C(0), C(1), "add", C(3), "sub", I(2), "mul", I(10), "gt"),         # int lane
        (C(6), C(6), "mul", F(0.5), "sub", C(6), "add", F(100.0), "lt"),    # double lane
        (C(0), C(6), "mul", C(4), F(0.25), "add", "sub", I(0), "ge"),       # mixed
        (C(0), C(4), "div", I(2), "ge"),                  # int / int incl. zero divisors
        (C(0), C(5), "div", C(1), "le"),                  # BOOLEAN divisor: half zeros
        (C(0), I(0), "div", I(0), "eq", "not"),           # always NULL
        (C(6), C(5), "div", F(1.0), "gt"),                # double / 0 = +-inf, NaN
        (C(1), I(7), "div", I(-3), "mul", C(1), "ne"),    # truncation toward zero
        (C(0), C(3), "add", I(0), "gt", C(1), I(0), "gt", "and"),
        (C(0), I(0), "gt", C(1), I(0), "gt", "or"),
        (C(0), I(0), "gt", "not"),
        (C(0), I(0), "gt", C(1), I(0), "gt", "or", "not", C(2), I(5), "lt", "and"),
        (C(0), C(1), C(2), "between"),
        (C(0), C(1), C(2), "between", "not"),
        (C(6), C(3), C(0), "between", C(4), I(0), "lt", "or"),
        (C(0),), (C(6),), (C(5), "not"),                  # bare truthiness
        (C(0), C(0), "sub", C(6), "mul", "not"),          # 0 * x: -0.0 is falsy
        deep_program(MAX_STACK),
        (C(0), I(0), "ge", C(0), I(0), "ge", "and") + ("not", "not"),
    ]


@pytest.mark.parametrize("nullable", [False, True], ids=["nonull", "nulls"])
def test_filter_flags_interpreter(sess, ops, nullable):
    cols = seven_page(N_TYPED, 33, nullable)
    rows, page = rows_of(cols), make_page(ops, cols)
    for prog in flags_programs():
        check_filter(sess, ops, cols, prog, None, rows, page, "flags")


def test_filter_flags_null_sides(sess, ops):
    """every (a, b) of {true, false, NULL}^2 under AND, OR, NOT, BETWEEN,
    each wrapped in NOT as well so a NULL result differs from false"""
    tri = [1, 0, None]
    vals = [(a, b, c) for a in tri for b in tri for c in tri] * 3
    cols = []
    for j in range(3):
        v = [r[j] for r in vals]
        cols.append(Col("i32", [POISON["i32"] if x is None else x for x in v],
                        [x is not None for x in v]))
    rows, page = rows_of(cols), make_page(ops, cols)
    for core in ((C(0), C(1), "and"), (C(0), C(1), "or"), (C(0), "not"),
                 (C(0), C(1), C(2), "between"), (C(0), C(1), "and", C(2), "or")):
        for tail in ((), ("not",), ("not", "not")):
            check_filter(sess, ops, cols, core + tail, None, rows, page, "flags")


def test_stack_depth_limits(sess, ops):
    """depth MAX_STACK runs (above), MAX_STACK+1 is TG_ERR_UNSUPPORTED,
    underflow and a two-value residue are TG_ERR_INVALID_ARG"""
    cols = seven_page(64, 1, False)
    page = make_page(ops, cols)
    assert stack_profile(deep_program(MAX_STACK))[0] == MAX_STACK
    assert stack_profile(deep_program(MAX_STACK + 1))[0] == MAX_STACK + 1
    run = lambda prog: (lambda: ops.filter_run(sess, ops.expr(*prog), page))   # noqa: E731
    expect_error(run(deep_program(MAX_STACK + 1)), TG_ERR_UNSUPPORTED, "depth")
    expect_error(run((C(0), "add")), TG_ERR_INVALID_ARG, "underflow")
    expect_error(run(("not",)), TG_ERR_INVALID_ARG, "underflow")
    expect_error(run((C(0), C(1))), TG_ERR_INVALID_ARG, "one value")
    expect_error(lambda: ops.filter_project(sess, None, [ops.expr(C(0), C(1))]),
                 TG_ERR_INVALID_ARG, "one value")


# --------------------------------------------------------------------------
# F2: rejected on the host before any upload or launch
# --------------------------------------------------------------------------
def _raw_expr(ops, items):
    """program with raw opcodes: (op, arg0) pairs"""
    insts = (ops.TgExprInst * len(items))()
    for i, (op, arg) in enumerate(items):
        insts[i].op, insts[i].arg0 = op, arg
    e = ops.TgExpr()
    e.insts, e.count, e._keepalive = insts, len(items), insts
    return e


def test_rejects_bad_column_index(sess, ops):
    cols = seven_page(64, 1, False)
    page = make_page(ops, cols)
    for bad in (len(cols), len(cols) + 100, -1, 2 ** 31 - 1):
        prog = (C(bad), I(1), "eq")
        expect_error(lambda: ops.filter_run(sess, ops.expr(*prog), page),
                     TG_ERR_INVALID_ARG, "column index")
        deep = (C(0), I(1), "eq", C(bad), I(1), "eq", "or")
        expect_error(lambda: ops.filter_run(sess, ops.expr(*deep), page),
                     TG_ERR_INVALID_ARG, "column index")
        if bad < 0:
            continue        # rejected at create already
        for f, p in ((prog, (C(0),)), (None, (C(bad),)), (None, (C(bad), I(1), "add"))):
            op = ops.filter_project(sess, ops.expr(*f) if f else None, [ops.expr(*p)])
            try:
                expect_error(lambda: op.add_input(page), TG_ERR_INVALID_ARG, "column index")
            finally:
                op.close()


def test_rejects_unimplemented_opcodes(sess, ops):
    page = make_page(ops, seven_page(64, 1, False))
    for opc in (ops.OP_IN, 18, 255, -1, 2 ** 31 - 1):
        raw = _raw_expr(ops, [(ops.OP_COL, 0), (ops.OP_COL, 1), (opc, 2)])
        expect_error(lambda: ops.filter_run(sess, raw, page), TG_ERR_UNSUPPORTED, "opcode")
        expect_error(lambda: ops.filter_project(sess, raw, [ops.expr(C(0))]),
                     TG_ERR_UNSUPPORTED, "opcode")
        expect_error(lambda: ops.filter_project(sess, None, [raw]),
                     TG_ERR_UNSUPPORTED, "opcode")


def test_rejects_varchar_in_expression(sess, ops):
    strs = Col("str", [b"ab", b"", b"c"] * 10)
    cols = [Col("i64", np.arange(30)), strs]
    page = make_page(ops, cols)
    for prog in ((C(1), I(1), "eq"), (C(0), C(1), "lt"), (C(1),),
                 (C(0), I(1), "eq", C(1), C(1), "eq", "and")):
        expect_error(lambda: ops.filter_run(sess, ops.expr(*prog), page),
                     TG_ERR_UNSUPPORTED, "VARCHAR")
    for f, p in (((C(1), I(1), "eq"), (C(0),)), (None, (C(1), I(1), "add")),
                 (None, (C(1), I(1), "le"))):
        op = ops.filter_project(sess, ops.expr(*f) if f else None, [ops.expr(*p)])
        try:
            expect_error(lambda: op.add_input(page), TG_ERR_UNSUPPORTED, "VARCHAR")
        finally:
            op.close()


# --------------------------------------------------------------------------
# cross-path agreement
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_three_paths_agree(sess, ops, kind):
    cols = [typed_col(kind, CHUNK + 77, 40, True)]
    rows, page = rows_of(cols), make_page(ops, cols)
    for const in (I(1), F(0.5)):
        base = (C(0), const, "le")
        exp = ref_filter(base, rows)
        for prog, path in ((base, "cmp"), (base + base + ("and",), "terms"),
                           (base + ("not", "not"), "flags")):
            assert path_of(prog) == path
            got = ops.filter_run(sess, ops.expr(*prog), page)
            assert got.tolist() == exp, (kind, const, path)


# --------------------------------------------------------------------------
# seeded random programs
# --------------------------------------------------------------------------
N_RANDOM = 997
# the first 64 seeds whose program keeps between 5 % and 95 % of random_page()
# (seeds whose program keeps nothing or everything were dropped)
RANDOM_SEEDS = (0, 1, 2, 3, 5, 7, 8, 11, 16, 18, 19, 20, 21, 23, 27, 28, 29, 30, 31, 32,
                35, 37, 38, 39, 40, 41, 42, 43, 44, 46, 47, 48, 51, 52, 53, 56, 59, 60,
                61, 62, 64, 65, 67, 68, 69, 70, 71, 72, 73, 76, 78, 79, 80, 82, 83, 85,
                86, 87, 88, 89, 90, 91, 92, 93)
_COL_BITS = {"i64": 8, "i32": 8, "date": 8, "i16": 13, "i8": 8, "bool": 1}


def random_program(seed):
    """a well-formed boolean postfix program of stack depth <= MAX_STACK over
    seven_page's columns. Every integer subexpression carries a bound on its
    bit length, kept <= 62, so the int lane cannot overflow; constants and
    cell values stay within +-2^31."""
    r = random.Random(seed)

    def leaf(want_float):
        if r.random() < 0.65:
            j = 6 if want_float else r.randrange(6)
            return [C(j)], 1, (None if j == 6 else _COL_BITS[KINDS[j]])
        if want_float:
            return [F(r.choice((-50.0, -0.25, 0.0, 0.5, 3.75, 20.0, 99.5)))], 1, None
        v = r.choice((-2 ** 31, -1000, -40, -3, -1, 0, 1, 2, 7, 50, 1000, 2 ** 31))
        return [I(v)], 1, max(abs(v).bit_length(), 1)

    def num(depth, room):
        """numeric expression: (items, stack need, int bit bound | None)"""
        if depth == 0 or room < 2 or r.random() < 0.3:
            return leaf(r.random() < 0.3)
        a, da, ba = num(depth - 1, room)
        b, db, bb = num(depth - 1, room - 1)
        op = r.choice(("add", "sub", "mul", "div"))
        if ba is None or bb is None:
            bits = None
        elif op == "mul":
            if ba + bb > 62:
                op = "sub"
                bits = max(ba, bb) + 1
            else:
                bits = ba + bb
        elif op == "div":
            bits = ba
        else:
            bits = max(ba, bb) + 1
        return a + b + [op], max(da, 1 + db), bits

    def boolean(depth, room):
        k = r.random()
        if depth == 0 or room < 3 or k < 0.45:
            a, da, _ = num(1 if depth == 0 else depth - 1, room)
            b, db, _ = num(1 if depth == 0 else depth - 1, room - 1)
            return a + b + [r.choice(CMPS)], max(da, 1 + db)
        if k < 0.6:
            a, da, _ = num(depth - 1, room)
            b, db, _ = num(0, room - 1)
            c, dc, _ = num(0, room - 2)
            return a + b + c + ["between"], max(da, 1 + db, 2 + dc)
        if k < 0.7:
            a, da = boolean(depth - 1, room)
            return a + ["not"], da
        a, da = boolean(depth - 1, room)
        b, db = boolean(depth - 1, room - 1)
        return a + b + [r.choice(("and", "or"))], max(da, 1 + db)

    prog, need = boolean(3, MAX_STACK)
    assert need <= MAX_STACK
    return tuple(prog)


@functools.lru_cache(None)
def random_page():
    cols = seven_page(N_RANDOM, 77, True)
    return cols, rows_of(cols)


@functools.lru_cache(None)
def random_reference(seed):
    """(program, kept positions); raises LeftInt64 if the reference does"""
    prog = random_program(seed)
    _, rows = random_page()
    return prog, ref_filter(prog, rows)


@pytest.mark.parametrize("block", range(4))
def test_random_programs(sess, ops, block):
    cols, rows = random_page()
    page = make_page(ops, cols)
    for seed in RANDOM_SEEDS[block::4]:
        prog, exp = random_reference(seed)
        got = ops.filter_run(sess, ops.expr(*prog), page)
        assert got.tolist() == exp, (seed, prog)


# --------------------------------------------------------------------------
# grid stride: n = TG_BLOCK * TG_MAX_BLOCKS + 257
# --------------------------------------------------------------------------
PERIOD = 1021        # prime: the pattern never lines up with wave, block or grid


@functools.lru_cache(None)
def grid_cols():
    """INTEGER and DOUBLE column of GRID_N rows, periodic in PERIOD rows, so
    the reference is evaluated over one period and tiled"""
    base = [typed_col("i32", PERIOD, 51, False), typed_col("f64", PERIOD, 52, False)]
    reps = -(-GRID_N // PERIOD)
    cols = [Col(c.kind, np.tile(c.values, reps)[:GRID_N]) for c in base]
    return base, cols


def tiled(per_period):
    reps = -(-GRID_N // PERIOD)
    return np.tile(np.asarray(per_period), reps)[:GRID_N]


GRID_FILTERS = (("cmp", (C(0), I(1), "ge")),
                ("terms", (C(0), I(1), "ge", C(1), F(1.0), "le", "and")),
                ("flags", (C(0), C(1), "add", F(1.5), "gt")))


@pytest.mark.parametrize("path,prog", GRID_FILTERS, ids=[p for p, _ in GRID_FILTERS])
def test_grid_stride_filters(sess, ops, path, prog):
    assert GRID_N > GRID_THREADS and path_of(prog) == path
    base, cols = grid_cols()
    keep = tiled([ref_keep(prog, row) for row in rows_of(base)])
    got = ops.filter_run(sess, ops.expr(*prog), make_page(ops, cols))
    assert np.array_equal(got, np.flatnonzero(keep).astype(np.int32))


GRID_PROJS = (("k_project", (C(0), C(1), "mul", F(0.5), "add")),
              ("k_gather", (C(1),)),
              ("k_proj_mulsub", (C(1), F(1.0), C(1), "sub", "mul")),
              ("k_proj_cmp_flag", (C(0), I(1), "ge")))


@pytest.mark.parametrize("name,prog", GRID_PROJS, ids=[p for p, _ in GRID_PROJS])
def test_grid_stride_projections(sess, ops, name, prog):
    """pure projection of every row: count == GRID_N > one grid of threads"""
    base, cols = grid_cols()
    ev, valid = ref_project(prog, "f64", rows_of(base), range(PERIOD))
    assert all(valid)
    op = ops.filter_project(sess, None, [ops.expr(*prog)], [ops.TG_DOUBLE])
    try:
        op.add_input(make_page(ops, cols))
        out = op.drain()[0][0]
    finally:
        op.close()
    assert out["valid"] is None or unpack_bits(out["valid"], GRID_N).all()
    exp = tiled(np.array(ev, np.float64))
    assert np.array_equal(out["values"].view(np.int64), exp.view(np.int64))


# --------------------------------------------------------------------------
# projection (FilterProjectOp)
# --------------------------------------------------------------------------
FILTERS = (None, (C(0), I(0), "ge"))     # pure projection | after a filter


def nonnull_f64_page(n, seed):
    r = np.random.default_rng(seed)
    return [Col("i64", r.integers(-50, 50, n)),
            Col("f64", np.round(r.uniform(0, 1000, n) * 100) / 100),
            Col("f64", np.round(r.uniform(0, 0.1, n) * 100) / 100),
            Col("i32", r.integers(-5, 6, n))]


@pytest.mark.parametrize("filt", FILTERS, ids=["pure", "filtered"])
def test_core_identity_every_width_with_nulls(sess, ops, filt):
    """k_gather<1|2|4|8>, validity carried"""
    cols = seven_page(N_TYPED, 61, True)
    check_project(sess, ops, [cols], filt, [((C(j),), k) for j, k in enumerate(KINDS)])


@pytest.mark.parametrize("filt", FILTERS, ids=["pure", "filtered"])
def test_core_interpreter_outputs(sess, ops, filt):
    """BIGINT and DOUBLE outputs of k_project over nullable and NULL-free pages"""
    projs = [((C(0), C(1), "mul", C(3), "sub"), "i64"),
             ((C(0), C(1), "mul", C(3), "sub"), "f64"),
             ((C(6), C(6), "mul", C(0), "add"), "f64"),
             ((C(6), F(0.75), "mul", C(4), "sub"), "i64"),    # double -> BIGINT truncates
             ((C(0), C(4), "div"), "i64"),
             ((C(6), C(5), "div"), "f64"),                    # +-inf and NaN
             ((C(0), I(0), "gt", C(1), I(0), "gt", "and"), "i64"),
             ((C(0), C(1), C(2), "between"), "f64")]
    for nullable in (True, False):
        check_project(sess, ops, [seven_page(N_TYPED, 62, nullable)], filt, projs)


@pytest.mark.parametrize("filt", FILTERS, ids=["pure", "filtered"])
def test_core_int_division_by_zero_is_null_without_bitmaps(sess, ops, filt):
    """F1: BIGINT a / b with zeros in b over NULL-free inputs: those rows are
    NULL, so the output needs a bitmap no input has"""
    r = np.random.default_rng(8)
    n = N_TYPED
    cols = [Col("i64", r.integers(-50, 50, n)), Col("i64", r.integers(-2, 3, n))]
    assert (cols[1].values == 0).sum() > 50
    check_project(sess, ops, [cols], filt,
                  [((C(0), C(1), "div"), "i64"), ((C(0), C(1), "div"), "f64"),
                   ((C(0), I(7), "add"), "i64")])


@pytest.mark.parametrize("filt", FILTERS, ids=["pure", "filtered"])
def test_projection_fast_paths_and_fallbacks(sess, ops, filt):
    """k_proj_cmp_flag and k_proj_mulsub, and the nullable / int-typed forms
    of the same expressions, which fall back to k_project"""
    n = N_TYPED
    cols = nonnull_f64_page(n, 70)
    r = np.random.default_rng(71)
    null = r.random(n) < 0.15
    ncols = [Col(c.kind, np.where(null, POISON[c.kind], c.values), ~null) if j else c
             for j, c in enumerate(cols)]
    projs = [((C(3), I(1), "ge"), "f64"), ((C(1), F(500.0), "lt"), "f64"),
             ((C(3), I(1), "ge"), "i64"),
             ((C(1), F(1.0), C(2), "sub", "mul"), "f64"),
             ((C(0), F(1.0), C(2), "sub", "mul"), "f64"),      # int-typed a
             ((C(1), F(1.0), C(3), "sub", "mul"), "f64"),      # int-typed b
             ((C(1), I(1), C(2), "sub", "mul"), "f64")]        # I64 constant
    check_project(sess, ops, [cols], filt, projs)
    check_project(sess, ops, [ncols], filt, projs)             # NULL rows stay NULL


def varchar_cols(n, seed):
    r = np.random.default_rng(seed)
    words = [b"", b"a", b"trino", b"", b"MI355X gfx950", b"xy" * 40]
    strs = [words[k] for k in r.integers(0, len(words), n)]
    null = r.random(n) < 0.1
    strs = [b"<poison>" if z else s for s, z in zip(strs, null)]
    return [Col("i32", np.arange(n)), Col("str", strs, ~null),
            Col("str", [b"%d" % i for i in range(n)])]


@pytest.mark.parametrize("count", VARCHAR_COUNTS)
def test_identity_varchar_counts(sess, ops, count):
    """run_gather_var; the last two counts exceed 2*FSCAN_CHUNK entries, so
    run_scan_i32 takes k_s32_chunk_sums / k_s32_chunks_serial / k_s32_offsets.
    Its recursive second level (> 8M entries) stays unreached."""
    projs = [((C(1),), "str"), ((C(2),), "str"), ((C(0),), "i32")]
    n = max(VARCHAR_COUNTS)
    check_project(sess, ops, [varchar_cols(n, 80)], (C(0), I(count), "lt"), projs)
    check_project(sess, ops, [varchar_cols(count, 81)], None, projs)


def test_core_filter_keeps_nothing(sess, ops):
    cols = seven_page(N_TYPED, 63, True)
    check_project(sess, ops, [cols], (C(0), I(1000), "gt"),
                  [((C(j),), k) for j, k in enumerate(KINDS)] +
                  [((C(0), C(1), "add"), "i64")])
    check_project(sess, ops, [varchar_cols(100, 82)], (C(0), I(0), "lt"),
                  [((C(1),), "str")])


def test_core_two_pages_through_one_operator(sess, ops):
    pages = [seven_page(N_TYPED, 64, True), seven_page(70, 65, False),
             seven_page(0, 66, True), seven_page(CHUNK + 5, 67, True)]
    check_project(sess, ops, pages, (C(0), C(1), "le"),
                  [((C(6),), "f64"), ((C(0), C(4), "div"), "i64"), ((C(3),), "i16")])


# --------------------------------------------------------------------------
# dynamic filter
# --------------------------------------------------------------------------
def df_bridge(sess, ops, keys, null=None):
    keys = np.asarray(keys, np.int64)
    bridge = ops.JoinBridge(sess)
    try:
        b = ops.hash_builder(sess, bridge, [ops.TG_BIGINT], [0], [0])
        try:
            ops.request_bitmap(bridge)
            v = None if null is None else [pack_bits(~np.asarray(null, bool))]
            b.add_input(ops.page_from_numpy([keys], valids=v))
            b.drain()
        finally:
            b.close()
    except Exception:
        bridge.close()
        raise
    return bridge


DF_FILTERS = (None, (C(1), I(0), "ge"), (C(1), I(-3), "ge", C(1), I(3), "le", "and"),
              (C(1), C(1), "mul", I(4), "le"))
DF_BUILDS = {"positive": [10, 11, 13, 40, 75, 76], "negative_mn": [-60, -59, -7, 0, 3, 64, 65]}


@pytest.mark.parametrize("build", sorted(DF_BUILDS))
@pytest.mark.parametrize("key_kind", ["i64", "i32", "date", "i16", "i8", "i64_nullable"])
def test_dynamic_filter(sess, ops, key_kind, build):
    """the bitmap after each flag kernel and alone (count == 0); probe keys
    below mn, above mx and NULL; F4: every integer key width is read at its
    own width"""
    bkeys = DF_BUILDS[build]
    r = np.random.default_rng(len(bkeys))
    n = CHUNK + 300
    kind = key_kind.split("_")[0]
    keys = r.integers(-100, 101, n)
    valid = None
    if key_kind.endswith("nullable"):
        null = r.random(n) < 0.1
        keys = np.where(null, bkeys[0], keys)      # poison: a key the bitmap holds
        valid = ~null
    cols = [Col(kind, keys, valid), typed_col("i32", n, 90, True), Col("i64", np.arange(n))]
    assert path_of(DF_FILTERS[1]) == "cmp" and path_of(DF_FILTERS[2]) == "terms"
    assert path_of(DF_FILTERS[3]) == "flags"
    members = set(bkeys)
    bridge = df_bridge(sess, ops, bkeys + [bkeys[0]], null=[False] * len(bkeys) + [True])
    try:
        for filt in DF_FILTERS:
            check_project(
                sess, ops, [cols], filt, [((C(2),), "i64"), ((C(0),), kind)],
                make_op=lambda f, pe, ot: ops.filter_project_df(sess, f, pe, ot, bridge, 0),
                keep=lambda row: row[0] is not None and row[0] in members)
    finally:
        bridge.close()


def test_dynamic_filter_rejects_bad_key_channel(sess, ops):
    """a DOUBLE or VARCHAR key channel, or one outside the page, is refused
    on the host (include/trino_gpu.h)"""
    bridge = df_bridge(sess, ops, [1, 2, 3])
    cols = [Col("f64", [1.0, 2.0]), Col("str", [b"1", b"2"]), Col("i64", [1, 2])]
    page = make_page(ops, cols)
    try:
        for ch, status in ((0, TG_ERR_UNSUPPORTED), (1, TG_ERR_UNSUPPORTED),
                           (3, TG_ERR_INVALID_ARG), (-1, TG_ERR_INVALID_ARG)):
            op = ops.filter_project_df(sess, None, [ops.expr(C(2))], [ops.TG_BIGINT],
                                       bridge, ch)
            try:
                expect_error(lambda: op.add_input(page), status, "dynamic filter key channel")
            finally:
                op.close()
    finally:
        bridge.close()


def test_core_dynamic_filter_and_varchar_leave_the_fused_path(sess, ops):
    """U1: the fused kernels know neither the dynamic filter nor VARCHAR, so
    such operators take the selection-vector path under TG_FP_FUSED=1 too"""
    n = 500
    cols = varchar_cols(n, 83)
    check_project(sess, ops, [cols], (C(0), I(77), "ge"), [((C(1),), "str"), ((C(0),), "i32")])
    bridge = df_bridge(sess, ops, [5, 6, 300, 301])
    try:
        for filt in (None, (C(0), I(6), "ge")):
            check_project(
                sess, ops, [cols], filt, [((C(0),), "i32"), ((C(2),), "str")],
                make_op=lambda f, pe, ot: ops.filter_project_df(sess, f, pe, ot, bridge, 0),
                keep=lambda row: row[0] in (5, 6, 300, 301))
    finally:
        bridge.close()


# --------------------------------------------------------------------------
# dictionary-aware filter
# --------------------------------------------------------------------------
def dict_case(kind, nd, n, seed, outer_nulls, dict_nulls):
    r = np.random.default_rng(seed)
    dv = typed_col(kind, nd, seed + 1, False).values
    ids = r.integers(0, nd, n).astype(np.int32)
    dvalid = None
    if dict_nulls:
        dvalid = r.random(nd) >= 0.3
        dvalid[0] = False
        dv = dv.copy()
        dv[~dvalid] = POISON[kind]
    ovalid = (r.random(n) >= 0.1) if outer_nulls else None
    flat_valid = None
    if dict_nulls or outer_nulls:
        flat_valid = np.ones(n, bool)
        if dvalid is not None:
            flat_valid &= dvalid[ids]
        if ovalid is not None:
            flat_valid &= ovalid
    return dv, ids, dvalid, ovalid, Col(kind, dv[ids], flat_valid)


DICT_PROGS = ((C(0), I(1), "ge"), (C(0), I(0), "ge", C(0), F(1.5), "le", "and"),
              (C(0), C(0), "mul", I(1), "eq"), (C(0), I(1), "lt", "not"))


def dict_page(ops, kind, dv, ids, dvalid, ovalid):
    page = ops.page_with_dict([(dv, ids)],
                              valids=[None if ovalid is None else pack_bits(ovalid)],
                              dict_valids=[None if dvalid is None else pack_bits(dvalid)])
    page.blocks[0].type = tg_type(ops, kind)
    page.blocks[0].dictionary.contents.type = tg_type(ops, kind)
    return page


@pytest.mark.parametrize("nulls", ["none", "outer", "dictionary", "both"])
@pytest.mark.parametrize("kind", KINDS)
def test_dictionary_filter(sess, ops, kind, nulls):
    """verdict per dictionary entry == the same filter over the decoded flat
    column == the reference. F3: a bitmap on the dictionary block and one on
    the dictionary itself both make rows NULL."""
    for nd, n in ((1, 70), (3, CHUNK + 9), (1000, CHUNK + 9)):
        if nd == 1 and nulls in ("dictionary", "both"):
            continue          # a one-entry dictionary with its entry NULL: below
        dv, ids, dvalid, ovalid, flat = dict_case(
            kind, nd, n, nd, nulls in ("outer", "both"), nulls in ("dictionary", "both"))
        rows = rows_of([flat])
        page = dict_page(ops, kind, dv, ids, dvalid, ovalid)
        flat_page = make_page(ops, [flat])
        for prog in DICT_PROGS:
            exp = ref_filter(prog, rows)
            assert ops.filter_run(sess, ops.expr(*prog), page).tolist() == exp, (nd, prog)
            assert ops.filter_run(sess, ops.expr(*prog), flat_page).tolist() == exp, (nd, prog)


def test_dictionary_all_entries_null_and_projection(sess, ops):
    """every entry NULL keeps nothing under a predicate and its negation; a
    decoded dictionary column projects with the folded bitmap"""
    dv = np.array([1, 1, 1], np.int64)
    ids = np.arange(200, dtype=np.int32) % 3
    page = dict_page(ops, "i64", dv, ids, np.zeros(3, bool), None)
    for prog in ((C(0), I(1), "eq"), (C(0), I(1), "eq", "not")):
        assert len(ops.filter_run(sess, ops.expr(*prog), page)) == 0
    dv, ids, dvalid, ovalid, flat = dict_case("i32", 5, 300, 3, True, True)
    op = ops.filter_project(sess, None, [ops.expr(C(0)), ops.expr(C(0), I(2), "mul")],
                            [ops.TG_INTEGER, ops.TG_BIGINT])
    try:
        op.add_input(dict_page(ops, "i32", dv, ids, dvalid, ovalid))
        out = op.drain()[0]
    finally:
        op.close()
    assert np.array_equal(unpack_bits(out[0]["valid"], 300), flat.valid)
    assert np.array_equal(unpack_bits(out[1]["valid"], 300), flat.valid)
    assert np.array_equal(out[0]["values"][flat.valid], flat.values[flat.valid])
    assert np.array_equal(out[1]["values"][flat.valid], 2 * flat.values[flat.valid].astype(np.int64))


@pytest.mark.parametrize("kind", KINDS)
def test_rle_block_null_free_value(sess, ops, kind):
    n = CHUNK + 1
    val = np.array([1], _NP[kind])
    page = ops.page_with_dict([(val, np.zeros(n, np.int32))])
    page.blocks[0].kind = 2                     # TG_BK_RLE
    page.blocks[0].ids = None
    page.blocks[0].type = tg_type(ops, kind)
    page.blocks[0].dictionary.contents.type = tg_type(ops, kind)
    rows = [(int(val[0]) if kind != "f64" else float(val[0]),)] * n
    for prog in ((C(0), I(1), "eq"), (C(0), I(1), "gt"), (C(0), F(0.5), "ge", "not", "not")):
        got = ops.filter_run(sess, ops.expr(*prog), page)
        assert got.tolist() == ref_filter(prog, rows), (kind, prog)


# --------------------------------------------------------------------------
# fused variant: the test_core_* subset in a fresh child under TG_FP_FUSED=1
# (the variable is read once per process)
# --------------------------------------------------------------------------
def test_core_flag_kernels_one_program_each(sess, ops):
    cols = seven_page(CHUNK + 70, 68, True)
    for filt in ((C(0), I(0), "ge"), (C(0), I(0), "ge", C(6), F(50.0), "lt", "and"),
                 (C(0), C(4), "div", I(0), "ne")):
        check_project(sess, ops, [cols], filt,
                      [((C(6),), "f64"), ((C(0), C(6), "mul"), "f64"), ((C(4),), "i8")])


def test_variant_fused():
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x",
           "-k", "test_core", "-p", "no:cacheprovider"]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, TG_FP_FUSED="1"), cwd=_ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
    except subprocess.TimeoutExpired:
        pytest.exit("filter matrix child (TG_FP_FUSED=1) hit its time limit: "
                    "nothing more is started on the GPU", returncode=3)
    if r.returncode < 0 or r.returncode >= 128:
        pytest.exit("filter matrix child (TG_FP_FUSED=1) ended on a signal "
                    f"(status {r.returncode}): nothing more is started on the "
                    f"GPU\n{r.stdout[-3000:]}", returncode=3)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:]
