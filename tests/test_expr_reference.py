"""Reference for the expression IR with IS_NULL, SELECT, COALESCE, a NULL
literal and IN lists, and the host-side checks of that IR (no GPU).

ref_eval2(prog, row, kinds) is a plain-Python postfix interpreter over the
items ops.expr takes: ('col', i) ('i64', v) ('f64', v) ('null', lane)
('in', [values]) and the op names. It returns (value, is_int, is_null) like
test_gpu_filter_matrix.ref_eval, with one difference: the lane of every stack
value is fixed by the program and the column kinds alone. ref_eval gives a
NULL cell the integer lane whatever its column; here a NULL cell of an 'f64'
column is in the double lane, so COALESCE(d, 1) / 2 divides as doubles on
every row.

 - is_null: 1 / 0 in the integer lane, never NULL;
 - select takes otherwise, cond, then: `then` iff cond is non-NULL and
   non-zero; coalesce takes a, b: a iff a is non-NULL. The result is in the
   integer lane iff both value operands are, else an integer operand is
   converted with float(i);
 - ('in', items): NULL for a NULL operand; an integer operand compares
   exactly, a double operand d as d == float(item), so NaN gives 0.

It is checked against ref_eval on the filter matrix's programs, against a
second reference made of Python closures over None, and by hand cases.
Also here: the library's validation through tg_expr_check, the set-form
choice through tg_expr_in_form, and the seeded random programs that
tests/test_gpu_expr_matrix.py runs on the GPU.
"""
import ctypes
import functools
import itertools
import math
import os
import random
import re

import pytest

from test_gpu_filter_matrix import (CMPS, FTERM_MAX, I64_MAX, I64_MIN, KINDS, MAX_STACK,
                                    N_TYPED, RANDOM_SEEDS, LeftInt64, _bool, _cmp, _fdiv,
                                    _is_col, _is_const, _kleene_and, _truthy, _tv,
                                    flags_programs, random_program, ref_eval, rows_of,
                                    seven_page, terms_programs)

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "trino_amd", "csrc")

TG_ERR_INVALID_ARG, TG_ERR_UNSUPPORTED = 1, 6
NEW_NAMES = ("is_null", "select", "coalesce")
FORM_MASK, FORM_BITMAP, FORM_SEARCH = 0, 1, 2


@functools.lru_cache(None)
def expr_constants():
    ev = open(os.path.join(_CSRC, "expr_eval.h")).read()
    oh = open(os.path.join(_CSRC, "operators.h")).read()

    def one(pat, text):
        m = re.search(pat, text)
        assert m, pat
        return int(m.group(1))

    return dict(IN_LIST_MAX=one(r"constexpr int IN_LIST_MAX = (\d+);", ev),
                EXPR_STACK_SLOTS=one(r"constexpr int EXPR_STACK_SLOTS = (\d+);", ev),
                IN_BITMAP_BITS=one(r"#define IN_BITMAP_BITS (\d+)", oh))


# the values the shapes here and in the GPU file assume, pinned below
IN_LIST_MAX = 4096
IN_BITMAP_BITS = 4096


def test_constants_are_the_sources():
    c = expr_constants()
    assert c["IN_LIST_MAX"] == IN_LIST_MAX and c["IN_BITMAP_BITS"] == IN_BITMAP_BITS
    assert c["EXPR_STACK_SLOTS"] == MAX_STACK == 6


# --------------------------------------------------------------------------
# reference
# --------------------------------------------------------------------------
def _pick(chosen, isint):
    """a SELECT / COALESCE result: `chosen` in the result's lane"""
    if chosen[2]:
        return (0, isint, True)
    return (chosen[0] if isint else float(chosen[0]), isint, False)


def ref_eval2(prog, row, kinds):
    st = []
    for it in prog:
        if isinstance(it, tuple):
            kind, v = it
            if kind == "col":
                isint = kinds[v] != "f64"
                x = row[v]
                st.append((0, isint, True) if x is None else (x, isint, False))
            elif kind == "i64":
                st.append((int(v), True, False))
            elif kind == "f64":
                st.append((float(v), False, False))
            elif kind == "null":
                assert v in (0, 1)
                st.append((0, v == 0, True))
            elif kind == "in":
                a = st.pop()
                if a[2]:
                    st.append(_bool(None))
                elif a[1]:
                    st.append(_bool(any(a[0] == int(x) for x in v)))
                else:
                    st.append(_bool(any(float(a[0]) == float(int(x)) for x in v)))
            else:
                raise ValueError(kind)
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
                r = (x + y if it == "add" else x - y if it == "sub" else
                     x * y if it == "mul" else _fdiv(x, y))
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
        elif it == "is_null":
            a = st.pop()
            st.append((1 if a[2] else 0, True, False))
        elif it == "select":
            then = st.pop()
            cond = st.pop()
            other = st.pop()
            take = (not cond[2]) and _truthy(cond)
            st.append(_pick(then if take else other, other[1] and then[1]))
        elif it == "coalesce":
            b = st.pop()
            a = st.pop()
            st.append(_pick(b if a[2] else a, a[1] and b[1]))
        else:
            raise ValueError(it)
    assert len(st) == 1, "malformed program"
    return st[0]


def ref_keep2(prog, row, kinds):
    v = ref_eval2(prog, row, kinds)
    return (not v[2]) and _truthy(v)


def stack_profile2(prog):
    """(max depth, final depth, underflowed)"""
    sp = mx = 0
    under = False
    for it in prog:
        if isinstance(it, tuple):
            sp += 0 if it[0] == "in" else 1
        elif it in ("not", "is_null"):
            pass
        elif it in ("between", "select"):
            sp -= 2
        else:
            sp -= 1
        mx = max(mx, sp)
        under |= sp < 1
    return mx, sp, under


def _is_in(it):
    return isinstance(it, tuple) and it[0] == "in"


def _match_term2(p, i, kinds):
    """items taken by the conjunction-path term at p[i:], 0 if none: the
    grammar of parse_fterms with the set term (integer column only) and the
    negated BETWEEN"""
    if i >= len(p) or not _is_col(p[i]):
        return 0
    if i + 1 < len(p) and _is_in(p[i + 1]):
        return 2 if kinds[p[i][1]] != "f64" else 0
    if (i + 6 < len(p) and _is_const(p[i + 1]) and p[i + 2] == "eq" and
            p[i + 3] == p[i] and _is_const(p[i + 4]) and p[i + 5] == "eq" and
            p[i + 6] == "or"):
        return 7
    if i + 3 < len(p) and _is_const(p[i + 1]) and _is_const(p[i + 2]) and p[i + 3] == "between":
        return 5 if i + 4 < len(p) and p[i + 4] == "not" else 4
    if i + 2 < len(p) and (_is_const(p[i + 1]) or _is_col(p[i + 1])) and p[i + 2] in CMPS:
        return 3
    return 0


def path_of2(prog, kinds):
    """the flag kernel run_filter picks: 'cmp', 'terms' or 'flags'"""
    p = list(prog)
    if len(p) == 3 and _is_col(p[0]) and _is_const(p[1]) and p[2] in CMPS:
        return "cmp"
    k = _match_term2(p, 0, kinds)
    if not k:
        return "flags"
    i, nt = k, 1
    while i < len(p):
        k = _match_term2(p, i, kinds)
        if not k or i + k >= len(p) or p[i + k] != "and":
            return "flags"
        i += k + 1
        nt += 1
    return "terms" if nt <= FTERM_MAX else "flags"


def in_form(items):
    """the representation tg_compile_expr picks for a list"""
    span = max(items) - min(items) + 1          # Python ints: no overflow
    return FORM_MASK if span <= 64 else FORM_BITMAP if span <= IN_BITMAP_BITS else FORM_SEARCH


C = lambda i: ("col", i)           # noqa: E731
I = lambda v: ("i64", v)           # noqa: E731
F = lambda v: ("f64", v)           # noqa: E731
NULL = lambda lane: ("null", lane)  # noqa: E731
IN = lambda *v: ("in", list(v))    # noqa: E731


def same(a, b):
    """two reference results agree on nullness, lane and value (-0.0 is not
    0.0, NaN is NaN)"""
    if a[2] or b[2]:
        return a[2] == b[2]
    if a[1] != b[1]:
        return False
    if a[1]:
        return a[0] == b[0] and isinstance(a[0], int) and isinstance(b[0], int)
    x, y = float(a[0]), float(b[0])
    if x != x or y != y:
        return x != x and y != y
    return x == y and math.copysign(1.0, x) == math.copysign(1.0, y)


# --------------------------------------------------------------------------
# (a) against ref_eval on the filter matrix's programs
# --------------------------------------------------------------------------
def test_agrees_with_filter_matrix_reference():
    """the old opcodes: the two references may differ only in the lane they
    give a NULL, which no old opcode can observe, so value, lane of a
    non-NULL result and nullness agree on every row"""
    rows = rows_of(seven_page(N_TYPED, 33, True))
    progs = [p for p, _ in terms_programs()] + list(flags_programs())
    progs += [random_program(s) for s in RANDOM_SEEDS]
    assert any(r[6] is None for r in rows)          # NULL DOUBLE cells are there
    for k, prog in enumerate(progs):
        for row in rows[k % 5::5]:
            try:
                old = ref_eval(prog, row)
            except LeftInt64:
                with pytest.raises(LeftInt64):
                    ref_eval2(prog, row, KINDS)
                continue
            assert same(old, ref_eval2(prog, row, KINDS)), (prog, row)


# --------------------------------------------------------------------------
# (b) against closures over None
# --------------------------------------------------------------------------
NAN = math.nan
# (cell, kind): NULL in either lane, then the values
OPERANDS = ((None, "i64"), (None, "f64"), (0, "i64"), (1, "i64"), (-1, "i64"),
            (2.5, "f64"), (NAN, "f64"), (-0.0, "f64"))
SET = (0, 1, 5)


def _lane(v, isint):
    return None if v is None else (v if isint else float(v))


def _eq(a, b):
    if a is None or b is None:
        return None
    if isinstance(a, int) and isinstance(b, int):
        return a == b
    return float(a) == float(b)


def _or3(a, b):
    if a is True or b is True:
        return True
    return None if a is None or b is None else False


# name -> (arity, program over columns 0.., closure(cells, all_int) -> value or None,
#          result is boolean)
def _constructs():
    member = lambda a: None if a is None else (a in SET)      # noqa: E731
    return {
        "is_null": (1, lambda k: (C(0), "is_null"), lambda v, ii: 1 if v[0] is None else 0, True),
        "coalesce": (2, lambda k: (C(0), C(1), "coalesce"),
                     lambda v, ii: _lane(v[0] if v[0] is not None else v[1], ii), False),
        "select": (3, lambda k: (C(0), C(1), C(2), "select"),
                   lambda v, ii: _lane(v[2] if (v[1] is not None and v[1] != 0) else v[0], ii),
                   False),
        "in": (1, lambda k: (C(0), IN(*SET)), lambda v, ii: member(v[0]), True),
        "not_in": (1, lambda k: (C(0), IN(*SET), "not"),
                   lambda v, ii: None if v[0] is None else not member(v[0]), True),
        "in_or_null": (1, lambda k: (C(0), IN(*SET), NULL(0), "or"),
                       lambda v, ii: _or3(member(v[0]), None), True),
        "nullif": (2, lambda k: (C(0), C(0), C(1), "eq", NULL(0 if k[0] != "f64" else 1), "select"),
                   lambda v, ii: None if _eq(v[0], v[1]) else v[0], False),
        "if": (3, lambda k: (C(2), C(0), C(1), "select"),       # IF(c0, c1, c2)
               lambda v, ii: _lane(v[1] if (v[0] is not None and v[0] != 0) else v[2], ii), False),
    }


@pytest.mark.parametrize("name", sorted(_constructs()))
def test_agrees_with_closures(name):
    arity, make, closure, boolean = _constructs()[name]
    value_operands = {"coalesce": (0, 1), "select": (0, 2), "if": (1, 2), "nullif": (0,)}
    for combo in itertools.product(OPERANDS, repeat=arity):
        row = tuple(c for c, _ in combo)
        kinds = tuple(k for _, k in combo)
        got = ref_eval2(make(kinds), row, kinds)
        all_int = all(kinds[j] != "f64" for j in value_operands.get(name, ()))
        exp = closure(row, all_int)
        if exp is None:
            assert got[2], (name, combo, got)
            continue
        if boolean:
            exp_t = (1 if exp else 0, True, False)
        else:
            exp_t = (exp, all_int, False)
        assert same(got, exp_t), (name, combo, got, exp_t)
        if not boolean:
            assert got[1] == all_int          # lane from the kinds, also when NULL
    # the lane of a NULL result is static too
    for combo in itertools.product(OPERANDS, repeat=arity):
        kinds = tuple(k for _, k in combo)
        if not boolean:
            got = ref_eval2(make(kinds), tuple(c for c, _ in combo), kinds)
            assert got[1] == all(kinds[j] != "f64" for j in value_operands[name])


# --------------------------------------------------------------------------
# (c) hand cases
# --------------------------------------------------------------------------
def case_chain(n):
    """CASE WHEN c0 = 1 THEN 10 WHEN c0 = 2 THEN 20 ... ELSE -1 END"""
    p = [I(-1)]
    for k in range(n, 0, -1):
        p += [C(0), I(k), "eq", I(10 * k), "select"]
    return tuple(p)


def test_hand_cases():
    ev = ref_eval2
    assert ev((C(0), IN(1, 2)), (None,), ("i64",))[2]                       # NULL IN -> NULL
    assert ev((C(0), IN(1, 2)), (None,), ("f64",))[2]
    assert ev((C(0), IN(0, 1)), (NAN,), ("f64",)) == (0, True, False)       # NaN IN -> 0
    assert ev((C(0), IN(0, 1)), (-0.0,), ("f64",)) == (1, True, False)      # -0.0 == 0
    assert ev((C(0), IN(3, 3, 1)), (3,), ("i32",)) == (1, True, False)      # duplicates
    assert ev((C(0), IN(2 ** 53 + 1)), (2 ** 53,), ("i64",)) == (0, True, False)   # exact
    assert ev((C(0), IN(2 ** 53 + 1)), (float(2 ** 53),), ("f64",)) == (1, True, False)
    assert ev((I(7), NULL(0), I(9), "select"), (), ()) == (7, True, False)  # NULL cond
    assert ev((I(7), I(0), I(9), "select"), (), ()) == (7, True, False)
    assert ev((I(7), F(NAN), I(9), "select"), (), ()) == (9, True, False)   # NaN is truthy
    assert ev((I(7), F(-0.0), I(9), "select"), (), ()) == (7, True, False)
    assert ev((I(7), I(1), F(0.5), "select"), (), ()) == (0.5, False, False)
    assert ev((I(7), I(0), F(0.5), "select"), (), ()) == (7.0, False, False)
    assert isinstance(ev((I(7), I(0), F(0.5), "select"), (), ())[0], float)
    # a CASE chain with 5 WHENs stays within the six slots
    chain = case_chain(5)
    assert stack_profile2(chain) == (3, 1, False) and MAX_STACK >= 3
    for v, exp in ((1, 10), (3, 30), (5, 50), (6, -1), (None, -1)):
        assert ev(chain, (v,), ("i32",)) == (exp, True, False)
    deep = (I(-1), C(0), C(0), C(0), C(0), "add", "add", "add", I(4), "eq", I(1), "select")
    assert stack_profile2(deep)[0] == 5
    # NULLIF(a, b) = a, a, b, EQ, NULL, SELECT
    nullif = (C(0), C(0), C(1), "eq", NULL(0), "select")
    assert ev(nullif, (3, 3), ("i64", "i64"))[2]
    assert ev(nullif, (3, 4), ("i64", "i64")) == (3, True, False)
    assert ev(nullif, (3, None), ("i64", "i64")) == (3, True, False)
    assert ev(nullif, (None, 3), ("i64", "i64"))[2]
    # COALESCE(d, 1) / 2 with d DOUBLE NULL divides as doubles
    half = (C(0), I(1), "coalesce", I(2), "div")
    assert ev(half, (None,), ("f64",)) == (0.5, False, False)
    assert ev(half, (None,), ("i64",)) == (0, True, False)
    assert ev(half, (3.0,), ("f64",)) == (1.5, False, False)
    assert ev((C(0), "is_null"), (None,), ("f64",)) == (1, True, False)
    assert ev((C(0), "is_null", "not"), (None,), ("f64",)) == (0, True, False)
    # x IN (1, NULL): true, else NULL
    in_null = (C(0), IN(1), NULL(0), "or")
    assert ev(in_null, (1,), ("i64",)) == (1, True, False)
    assert ev(in_null, (2,), ("i64",))[2]


# --------------------------------------------------------------------------
# validation, through the host-only tg_expr_check
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from trino_amd import ops
    return ops


def raw_expr(ops, items):
    """(op, arg0[, i64]) triples as they are"""
    insts = (ops.TgExprInst * len(items))()
    for i, it in enumerate(items):
        insts[i].op, insts[i].arg0 = it[0], it[1]
        if len(it) > 2:
            insts[i].imm.i64 = it[2]
    e = ops.TgExpr()
    e.insts, e.count, e._keepalive = insts, len(items), insts
    return e


def check_status(ops, e):
    """(status, message) of tg_expr_check"""
    import trino_amd
    try:
        ops.expr_check(e)
    except trino_amd.TrinoGpuError as err:
        m = re.match(r"status (\d+): (.*)", str(err), re.S)
        return int(m.group(1)), m.group(2)
    return 0, ""


def test_validation_table(ops):
    o = ops
    col, lst, item, null = (o.OP_COL, 0), o.OP_IN_LIST, (o.OP_IN_ITEM, 0, 5), o.OP_CONST_NULL
    bad = [
        ([col, (lst, 0)], TG_ERR_INVALID_ARG, "IN list"),                     # k < 1
        ([col, (lst, -3), item], TG_ERR_INVALID_ARG, "IN list"),
        ([col, (lst, 2), item], TG_ERR_INVALID_ARG, "runs past"),             # past the end
        ([col, (lst, 1)], TG_ERR_INVALID_ARG, "runs past"),
        ([col, (lst, 2 ** 31 - 1), item], TG_ERR_UNSUPPORTED, "IN list"),
        ([col, (lst, 2), item, col, (o.OP_EQ, 0)], TG_ERR_INVALID_ARG, "not an IN item"),
        ([col, item], TG_ERR_INVALID_ARG, "outside an IN list"),              # stray item
        ([item], TG_ERR_INVALID_ARG, "outside an IN list"),
        ([col, (lst, 1), item, item], TG_ERR_INVALID_ARG, "outside an IN list"),
        ([(null, 2)], TG_ERR_INVALID_ARG, "lane"),
        ([(null, -1)], TG_ERR_INVALID_ARG, "lane"),
        ([col, (lst, IN_LIST_MAX + 1)] + [item] * (IN_LIST_MAX + 1), TG_ERR_UNSUPPORTED, "IN list"),
        ([(o.OP_IS_NULL, 0)], TG_ERR_INVALID_ARG, "underflow"),
        ([(lst, 1), item], TG_ERR_INVALID_ARG, "underflow"),
        ([col, (o.OP_COALESCE, 0)], TG_ERR_INVALID_ARG, "underflow"),
        ([col, col, (o.OP_SELECT, 0)], TG_ERR_INVALID_ARG, "underflow"),
        ([col, col, (o.OP_IS_NULL, 0)], TG_ERR_INVALID_ARG, "one value"),
        ([col, (null, 0)], TG_ERR_INVALID_ARG, "one value"),
        ([(null, 0)] * 7 + [(o.OP_COALESCE, 0)] * 6, TG_ERR_UNSUPPORTED, "depth"),
        ([(o.OP_COL, -1), (o.OP_IS_NULL, 0)], TG_ERR_INVALID_ARG, "column index"),
    ]
    for opc in list(range(17, 32)) + [38, 255, -1, 2 ** 31 - 1]:
        bad.append(([col, col, (opc, 2)], TG_ERR_UNSUPPORTED, "opcode"))
    for items, status, word in bad:
        got, msg = check_status(o, raw_expr(o, items))
        assert got == status and word in msg, (items[:6], got, msg)
    good = [
        [col, (lst, 1), item],
        [col, (lst, IN_LIST_MAX)] + [item] * IN_LIST_MAX,
        [col, (lst, 3), item, item, (o.OP_IN_ITEM, 77, -9), (o.OP_NOT, 0)],   # arg0 of an item is not read
        [(null, 0)], [(null, 1), (o.OP_IS_NULL, 0)],
        [(null, 0)] * 6 + [(o.OP_COALESCE, 0)] * 5,                           # depth 6
        [col, col, col, (o.OP_SELECT, 0)],
    ]
    for items in good:
        assert check_status(o, raw_expr(o, items)) == (0, ""), items[:6]
    # an item whose imm looks like a column index or a divisor is data
    e = o.expr(C(0), IN(-1, 2 ** 31 - 1, 0))
    assert check_status(o, e) == (0, "")
    # the same text as the operators give: the python names go through too
    assert check_status(o, o.expr(*case_chain(5))) == (0, "")
    assert check_status(o, o.expr(C(0), "select"))[0] == TG_ERR_INVALID_ARG
    # the length limit counts operations, not items
    long_ok = [C(0), IN(*range(300))] + [C(0), I(1), "eq", "or"] * 31
    assert len(long_ok) < 128 and check_status(o, o.expr(*long_ok)) == (0, "")
    too_long = [C(0), I(1), "eq"] + [C(0), I(1), "eq", "or"] * 32
    st, msg = check_status(o, o.expr(*too_long))
    assert st == TG_ERR_UNSUPPORTED and "too long" in msg


def test_expr_builder_expands_in(ops):
    e = ops.expr(C(2), IN(7, -1, 7), "not", NULL(1), "coalesce")
    got = [(e.insts[i].op, e.insts[i].arg0, e.insts[i].imm.i64) for i in range(e.count)]
    assert got == [(ops.OP_COL, 2, 0), (ops.OP_IN_LIST, 3, 0), (ops.OP_IN_ITEM, 0, 7),
                   (ops.OP_IN_ITEM, 0, -1), (ops.OP_IN_ITEM, 0, 7), (ops.OP_NOT, 0, 0),
                   (ops.OP_CONST_NULL, 1, 0), (ops.OP_COALESCE, 0, 0)]
    assert ops.OP_IN == 17
    assert (ops.OP_IS_NULL, ops.OP_SELECT, ops.OP_COALESCE, ops.OP_CONST_NULL,
            ops.OP_IN_LIST, ops.OP_IN_ITEM) == (32, 33, 34, 35, 36, 37)


# --------------------------------------------------------------------------
# set forms
# --------------------------------------------------------------------------
def form_cases():
    b = IN_BITMAP_BITS
    return [
        ([5], FORM_MASK), ([0, 63], FORM_MASK), ([-40, 23], FORM_MASK),       # span 64
        ([0, 64], FORM_BITMAP), ([-40, 24], FORM_BITMAP),                     # span 65
        ([10, 10 + b - 1], FORM_BITMAP), ([10, 10 + b], FORM_SEARCH),         # BITS, BITS + 1
        ([I64_MIN, I64_MAX], FORM_SEARCH), ([I64_MIN, I64_MIN + 63], FORM_MASK),
        ([I64_MAX - 64, I64_MAX], FORM_BITMAP), ([I64_MAX, I64_MIN, 0], FORM_SEARCH),
        ([3, 3, 3], FORM_MASK), ([64, 0, 64, 0], FORM_BITMAP),                # duplicates, unsorted
        ([49, 14, 23, 45, 19, 3, 36, 9], FORM_MASK),                          # Q16's sizes
        (list(range(0, 4096 * 1000, 1000)), FORM_SEARCH),
    ]


def test_set_form_model_and_host_choice():
    from trino_amd import _lib
    _lib.tg_expr_in_form.restype = ctypes.c_int32
    _lib.tg_expr_in_form.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    for items, form in form_cases():
        assert in_form(items) == form, items[:4]
        arr = (ctypes.c_int64 * len(items))(*items)
        assert _lib.tg_expr_in_form(arr, len(items)) == form, items[:4]
    assert _lib.tg_expr_in_form(None, 0) == -1


# --------------------------------------------------------------------------
# seeded random programs (run on the GPU by tests/test_gpu_expr_matrix.py)
# --------------------------------------------------------------------------
N_PROGRAMS = 96
N_RANDOM_ROWS = 499
_INT_CONSTS = (-1000, -40, -3, -1, 0, 1, 2, 7, 50, 1000)
_F64_CONSTS = (-50.0, -0.25, 0.0, 0.5, 3.75, 20.0, 99.5)


def _random_program(seed):
    """a boolean postfix program of depth <= MAX_STACK over seven_page's
    columns; shape 0 is the bare compare, shape 1 a conjunction of terms"""
    r = random.Random(seed)

    def in_list():
        k = r.choice((1, 2, 3, 8, 8, 40))
        lo, hi = r.choice(((-5, 5), (-100, 100), (-100, 100), (-3000, 3000), (-10 ** 6, 10 ** 6)))
        return ("in", [r.randint(lo, hi) for _ in range(k)])

    def term():
        k = r.random()
        if k < 0.45:
            return [C(r.randrange(6)), in_list()]
        if k < 0.6:
            return [C(r.randrange(7)), I(-60), I(r.choice((0, 40))), "between"] + \
                   (["not"] if r.random() < 0.5 else [])
        if k < 0.8:
            return [C(r.randrange(7)), r.choice((I(r.choice(_INT_CONSTS)), F(r.choice(_F64_CONSTS)))),
                    r.choice(CMPS)]
        return [C(r.randrange(7)), C(r.randrange(7)), r.choice(CMPS)]

    def leaf():
        k = r.random()
        if k < 0.6:
            return [C(r.randrange(7))], 1
        if k < 0.75:
            return [I(r.choice(_INT_CONSTS))], 1
        if k < 0.88:
            return [F(r.choice(_F64_CONSTS))], 1
        return [NULL(r.randrange(2))], 1

    def num(depth, room):
        """numeric expression of at most 2^depth leaves: (items, stack need)"""
        if depth == 0 or room < 2 or r.random() < 0.3:
            return leaf()
        k = r.random()
        if k < 0.3 and room >= 3:
            o, do = num(depth - 1, room)
            c, dc = boolean(1, room - 1)
            t, dt = num(depth - 1, room - 2)
            return o + c + t + ["select"], max(do, 1 + dc, 2 + dt)
        a, da = num(depth - 1, room)
        b, db = num(depth - 1, room - 1)
        op = "coalesce" if k < 0.55 else r.choice(("add", "sub", "mul", "div"))
        return a + b + [op], max(da, 1 + db)

    def boolean(depth, room):
        k = r.random()
        if depth == 0 or room < 3 or k < 0.3:
            a, da = num(min(depth, 2), room)
            b, db = num(min(depth, 1), room - 1)
            return a + b + [r.choice(CMPS)], max(da, 1 + db)
        if k < 0.45:
            a, da = num(2, room)
            return a + [in_list()], da
        if k < 0.57:
            a, da = num(2, room)
            return a + ["is_null"], da
        if k < 0.65:
            a, da = num(1, room)
            b, db = num(0, room - 1)
            c, dc = num(0, room - 2)
            return a + b + c + ["between"], max(da, 1 + db, 2 + dc)
        if k < 0.75:
            a, da = boolean(depth - 1, room)
            return a + ["not"], da
        a, da = boolean(depth - 1, room)
        b, db = boolean(depth - 1, room - 1)
        return a + b + [r.choice(("and", "or"))], max(da, 1 + db)

    shape = seed % 8
    if shape == 0:
        return (C(r.randrange(7)), r.choice((I(r.choice(_INT_CONSTS)), F(r.choice(_F64_CONSTS)))),
                r.choice(CMPS))
    if shape in (1, 2):
        n = r.choice((1, 2, 3, FTERM_MAX))
        prog = term()
        for _ in range(n - 1):
            prog += term() + ["and"]
        return tuple(prog)
    prog, need = boolean(3, MAX_STACK)
    assert need <= MAX_STACK
    return tuple(prog)


@functools.lru_cache(None)
def random_rows():
    cols = seven_page(N_RANDOM_ROWS, 177, True)
    return cols, rows_of(cols)


@functools.lru_cache(None)
def random_case(index):
    """(program, kept positions of random_rows()) of the index-th program: a
    program whose reference leaves int64 on some row is generated again from
    the next seed of its own series, never dropped"""
    _, rows = random_rows()
    for attempt in range(50):
        prog = _random_program(index + 8 * 1000 * attempt)
        try:
            return prog, [i for i, row in enumerate(rows) if ref_keep2(prog, row, KINDS)]
        except LeftInt64:
            continue
    raise AssertionError(f"no program for index {index}")


def _ops_of(prog):
    out = set()
    for it in prog:
        if isinstance(it, tuple):
            if it[0] in ("null", "in"):
                out.add(it[0])
        elif it in NEW_NAMES:
            out.add(it)
    return out


def test_random_programs_cover_the_ground():
    cases = [random_case(k) for k in range(N_PROGRAMS)]
    assert len(cases) == N_PROGRAMS and len({p for p, _ in [(tuple(map(repr, c[0])), 0) for c in cases]}) > N_PROGRAMS * 3 // 4
    for name in NEW_NAMES + ("null", "in"):
        n = sum(name in _ops_of(p) for p, _ in cases)
        assert n * 10 >= N_PROGRAMS, (name, n)
    paths = [path_of2(p, KINDS) for p, _ in cases]
    for path in ("cmp", "terms", "flags"):
        assert paths.count(path) >= 4, (path, paths.count(path))
    for prog, keep in cases:
        mx, final, under = stack_profile2(prog)
        assert mx <= MAX_STACK and final == 1 and not under, prog
    # the programs tell rows apart: most keep some rows and drop some
    mixed = sum(0 < len(keep) < N_RANDOM_ROWS for _, keep in cases)
    assert mixed * 2 >= N_PROGRAMS, mixed


def test_random_programs_pass_the_library_check(ops):
    for k in range(N_PROGRAMS):
        prog, _ = random_case(k)
        assert check_status(ops, ops.expr(*prog)) == (0, ""), prog
