"""Join filter parity matrix: ops.lookup_join(..., filter=) for all four join
types plus the lookup-outer operator, against tests/test_join_filter_reference
.py (ref_join_filtered on ref_join's candidate order and the filter matrix's
ref_keep; ref_join_filtered_vec where candidates exceed ~10^4).

Contract checked, bit-exactly and in list order, no tolerances:
 - the probe operator emits the unfiltered inner output with the pairs that
   fail the filter (zero or NULL) removed and nothing else moved; under
   join_type 1 | 3 a probe row left without a pair emits one NULL-build row
   at its place;
 - under join_type 2 | 3 only surviving pairs are recorded, so the
   lookup-outer operator emits every build row in no surviving pair.
Under TG_JOIN_CSR=0 the pairs of one probe row compare as a set, as in the
join matrices.

Unless a case cannot by construction (constant filters, empty sides, fewer
than six candidates), it first asserts on the reference that it holds a probe
row with several candidates of which some survive and some fail, a probe row
whose candidates all fail, and a pair whose filter result is NULL.

Sizes are the smallest that reach each edge: the wave (63 | 64 | 65), more
than GRID_THREADS candidates for the second stride of the per-pair kernels,
and JSCAN_CHUNK - 1 | +0 | +1 | 2x + 1 candidates and probe rows for
run_scan_counts, the only scan the filter step runs (over the keep flags of
the pairs, and under LEFT / FULL over the survivor counts and the
survivor-less flags of the probe rows).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_filter_matrix import ref_eval
from test_gpu_join_matrix import (  # noqa: F401  (sess, ops, partitioned: fixtures)
    GENERIC, GRID_THREADS, JSCAN_CHUNK, ORDER, OVERFLOW_N, POISON_I, Col, build_bridge,
    concat_cols, generic_tables, key_of, keys_of, make_page, nullable, ops,
    output_cols, partitioned, ref_join, ref_join_vec, rng, sess, split_pages, tg_types)
from test_gpu_outer_join_matrix import check_inner, emit_outer
from test_join_filter_reference import ref_join_filtered, ref_join_filtered_vec
from test_outer_join_reference import ref_unmatched

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TG_ERR_INVALID_ARG, TG_ERR_UNSUPPORTED = 1, 6
ALL_TYPES = [0, 1, 2, 3]
JT_IDS = ["inner", "left", "right", "full"]
MAX_STACK = 6

C = lambda i: ("col", i)           # noqa: E731
I = lambda v: ("i64", v)           # noqa: E731
F = lambda v: ("f64", v)           # noqa: E731
TRUE, FALSE = (I(1),), (I(0),)


# --------------------------------------------------------------------------
# runner
# --------------------------------------------------------------------------
def cells(cols):
    return [tuple(c.cell(i) for c in cols) for i in range(len(cols[0]))]


def assert_coverage(op, keep, null):
    """candidate probe rows, keep flags and NULL-result flags of a case"""
    op, keep, null = np.asarray(op, np.int64), np.asarray(keep, bool), np.asarray(null, bool)
    m = int(op.max()) + 1 if len(op) else 0
    c, k = np.bincount(op, minlength=m), np.bincount(op[keep], minlength=m)
    assert ((c >= 2) & (k > 0) & (k < c)).any(), "no probe row kept some and lost some"
    assert ((c >= 1) & (k == 0)).any(), "no probe row lost every candidate"
    assert null.any(), "no pair with a NULL filter result"


def py_reference(build_cols, probe_cols, bkeys, pkeys, prog, outer, cover):
    brows, prows = cells(build_cols), cells(probe_cols)
    if cover:
        cands = ref_join(keys_of(build_cols, bkeys), keys_of(probe_cols, pkeys), False)
        vals = [ref_eval(prog, prows[i] + brows[r]) for i, r in cands]
        assert_coverage([i for i, _ in cands], [not v[2] and v[0] != 0 for v in vals],
                        [v[2] for v in vals])
    pairs, un = ref_join_filtered(brows, prows, bkeys, pkeys, prog, outer)
    eop = np.array([p for p, _ in pairs], np.int64)
    eob = np.array([-1 if b is None else b for _, b in pairs], np.int64)
    return eop, eob, np.array(un, np.int64)


def vec_reference(build_cols, probe_cols, bkeys, pkeys, pred, outer, cover):
    """pred(op, ob) -> (keep, null) over candidate index arrays"""
    bk, pk = build_cols[bkeys[0]], probe_cols[pkeys[0]]
    args = (bk.values, bk.valid, pk.values, pk.valid)
    if cover:
        op, ob = ref_join_vec(*args)
        assert_coverage(op, *pred(op, ob))
    return ref_join_filtered_vec(*args, lambda op, ob: pred(op, ob)[0], outer)


def run_probe(sess, ops, bridge, probe_pages, pkeys, pout, join_type, prog):
    op = ops.lookup_join(sess, bridge, tg_types(ops, probe_pages[0]), pkeys, pout,
                         join_type=join_type,
                         filter=None if prog is None else ops.expr(*prog))
    try:
        for p in probe_pages:
            op.add_input(make_page(ops, p))
        return op.drain()
    finally:
        op.close()


def filtered_case(sess, ops, build_pages, bkeys, bout, probes, pkeys, pout, join_type,
                  progs, preds=None, order=ORDER, cover=True):
    """build; one operator per entry of `probes` (lists of pages) with the
    matching entry of `progs`, each checked against the reference; under
    join_type 2 | 3 the lookup-outer operator against the build rows in no
    surviving pair of any of them. preds: numpy twins of progs (vectorised
    reference) or None (Python reference). Returns the unmatched rows."""
    build_cols = concat_cols(build_pages)
    outer = join_type in (1, 3)
    matched_none = np.ones(len(build_cols[0]), bool)
    refs = []
    for k, probe_pages in enumerate(probes):
        probe_cols = concat_cols(probe_pages)
        if preds is None:
            eop, eob, un = py_reference(build_cols, probe_cols, bkeys, pkeys, progs[k],
                                        outer, cover)
        else:
            eop, eob, un = vec_reference(build_cols, probe_cols, bkeys, pkeys, preds[k],
                                         outer, cover)
        keep = np.zeros(len(build_cols[0]), bool)
        keep[un] = True
        matched_none &= keep
        refs.append((eop, eob))
    bridge = build_bridge(sess, ops, build_pages, bkeys, bout)
    try:
        for k, probe_pages in enumerate(probes):
            pages = run_probe(sess, ops, bridge, probe_pages, pkeys, pout, join_type,
                              progs[k])
            check_inner(ops, pages, probe_pages, pkeys, pout, build_cols, bkeys, bout,
                        outer, order, refs[k])
        unmatched = np.flatnonzero(matched_none)
        if join_type >= 2:
            pout_cols = [probes[0][0][ch] for ch in pout]
            emit_outer(sess, ops, bridge, build_cols, bout, pout_cols, unmatched)
        return unmatched, refs
    finally:
        bridge.close()


# --------------------------------------------------------------------------
# tables
# --------------------------------------------------------------------------
NP_RICH = 7          # probe channels of rich_tables: build channel b is NP_RICH + b


def rich_tables(seed=5, nb=300, m=257):
    """build [key, y, d, f, hidden, row], probe [key, x, lo, hi, g, hidden,
    row]; about three build rows per key, half the probe hits, NULLs over
    poison in every filter operand"""
    r = rng(seed)
    bk = key_of(r.integers(0, nb // 3, nb))
    brow, prow = np.arange(nb), np.arange(m)
    build = [nullable("i64", bk, brow % 41 == 7),
             nullable("i64", r.integers(-2, 4, nb), r.random(nb) < 0.15, POISON_I),
             nullable("date", r.integers(0, 20, nb), r.random(nb) < 0.1, 5),
             nullable("f64", r.integers(-4, 8, nb) * 0.5, r.random(nb) < 0.1, 0.5),
             nullable("i16", r.integers(-3, 4, nb) * 1000, r.random(nb) < 0.15, 0),
             Col("i64", brow)]
    pk = key_of(10 * nb + 7 + prow)
    pk[0::2] = r.choice(bk, len(pk[0::2]))
    lo = r.integers(0, 12, m)
    probe = [nullable("i64", pk, prow % 37 == 5),
             nullable("i64", r.integers(-2, 4, m), r.random(m) < 0.15, POISON_I),
             nullable("i32", lo, r.random(m) < 0.1, 0),
             Col("i32", lo + r.integers(0, 9, m)),
             nullable("f64", r.integers(-4, 8, m) * 0.5, r.random(m) < 0.1, 0.5),
             nullable("i8", r.integers(-3, 4, m), r.random(m) < 0.15, 0),
             Col("i64", prow)]
    assert len(probe) == NP_RICH
    return build, probe


B = lambda b: C(NP_RICH + b)       # noqa: E731
RICH_FILTERS = {
    "ne_q21": (C(1), B(1), "ne"),
    "between": (B(2), C(2), C(3), "between"),
    "mixed_double_bigint": (C(1), B(3), "lt"),
    "mixed_arith": (C(4), B(1), "add", B(3), C(1), "mul", "ge"),
    "int_div_zero": (C(1), B(1), "div", I(0), "ge"),
    "not_eq_over_null": (C(1), B(1), "eq", "not"),
    "or_true_dominates_null": (C(1), B(1), "eq", C(2), I(5), "lt", "or"),
    "hidden_channels": (C(5), B(4), I(1000), "div", "le"),
}
RICH_BOUT, RICH_POUT = [1, 3, 5], [1, 4, 6]


@pytest.mark.parametrize("join_type", ALL_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("name", list(RICH_FILTERS))
def test_filters(sess, ops, name, join_type):
    """every filter form; 'hidden_channels' names a build channel that is
    neither key nor output and a probe channel that is no output"""
    build, probe = rich_tables()
    filtered_case(sess, ops, [build], [0], RICH_BOUT, [[probe]], [0], RICH_POUT,
                  join_type, [RICH_FILTERS[name]])


def _run_child(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x",
           "-k", "test_filters and (ne_q21 or between)", "-p", "no:cacheprovider"]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, **env), cwd=_ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
    except subprocess.TimeoutExpired:
        pytest.exit(f"join filter matrix child {env} hit its time limit: nothing "
                    "more is started on the GPU", returncode=3)
    if r.returncode < 0 or r.returncode >= 128:
        pytest.exit(f"join filter matrix child {env} ended on a signal "
                    f"(status {r.returncode}): nothing more is started on the "
                    f"GPU\n{r.stdout[-3000:]}", returncode=3)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:]


def test_variant_kv_table():
    """core filters under TG_JOIN_KV=1: full list-order contract"""
    _run_child({"TG_JOIN_KV": "1"})


def test_variant_legacy_table():
    """core filters under TG_JOIN_CSR=0: pairs of each probe row as a set"""
    _run_child({"TG_JOIN_CSR": "0"})


# --------------------------------------------------------------------------
# every fixed width on both sides
# --------------------------------------------------------------------------
WIDTHS = ("i8", "i16", "i32", "date", "i64", "f64", "bool")


@pytest.mark.parametrize("join_type", [1, 2], ids=["left", "right"])
@pytest.mark.parametrize("kind", WIDTHS)
def test_every_width_on_both_sides(sess, ops, kind, join_type):
    """probe.v <> build.v with both operands of `kind` (BOOLEAN cells are one
    byte, the page and the builder are told TG_BOOLEAN)"""
    r = rng(3)
    nb, m = 200, 129
    ckind = "i8" if kind == "bool" else kind
    dom = {"i8": 50, "i16": 10000, "i32": 10 ** 9, "date": 7000, "i64": 2 ** 60,
           "f64": 0.5, "bool": 1}[kind]
    small = (0, 2) if kind == "bool" else (-1, 2)
    bk = key_of(r.integers(0, nb // 3, nb))
    build = [Col("i64", bk),
             nullable(ckind, r.integers(*small, nb) * dom, r.random(nb) < 0.15, dom),
             Col("i64", np.arange(nb))]
    pk = key_of(r.integers(0, nb // 3 + 20, m))
    probe = [Col("i64", pk),
             nullable(ckind, r.integers(*small, m) * dom, r.random(m) < 0.15, dom),
             Col("i64", np.arange(m))]
    prog = (C(1), C(3 + 1), "ne")
    build_cols, probe_cols = build, probe
    eop, eob, un = py_reference(build_cols, probe_cols, [0], [0], prog,
                                join_type == 1, True)

    def typed(cols):
        t = tg_types(ops, cols)
        if kind == "bool":
            t[1] = ops.TG_BOOLEAN
        return t

    def page(cols):
        p = make_page(ops, cols)
        p.blocks[1].type = typed(cols)[1]
        return p

    bridge = ops.JoinBridge(sess)
    try:
        b = ops.hash_builder(sess, bridge, typed(build), [0], [0, 2])
        b.add_input(page(build))
        b.drain()
        b.close()
        op = ops.lookup_join(sess, bridge, typed(probe), [0], [0, 2],
                             join_type=join_type, filter=ops.expr(*prog))
        try:
            op.add_input(page(probe))
            pages = op.drain()
        finally:
            op.close()
        check_inner(ops, pages, [probe], [0], [0, 2], build, [0], [0, 2],
                    join_type == 1, ORDER, (eop, eob))
        if join_type == 2:
            emit_outer(sess, ops, bridge, build, [0, 2], [probe[0], probe[2]], un)
    finally:
        bridge.close()


# --------------------------------------------------------------------------
# constant filters
# --------------------------------------------------------------------------
def _same_pages(got, ref):
    assert len(got) == len(ref)
    for gp, rp in zip(got, ref):
        assert len(gp) == len(rp)
        for g, r in zip(gp, rp):
            assert g["type"] == r["type"]
            assert g["values"].tobytes() == r["values"].tobytes()
            assert (g["valid"] is None) == (r["valid"] is None)
            if g["valid"] is not None:             # the n bits the page owns
                n = len(g["values"])
                bits = [np.unpackbits(x["valid"].view(np.uint8), bitorder="little")[:n]
                        for x in (g, r)]
                assert np.array_equal(*bits)


@pytest.mark.parametrize("join_type", ALL_TYPES, ids=JT_IDS)
def test_constant_true_is_byte_identical(sess, ops, join_type):
    """filter TRUE and filter=None against the unfiltered operator on the
    same built table, raw pages; and the same unmatched rows afterwards"""
    build, probe = rich_tables(seed=8)
    pages = split_pages(probe, [100, 0, len(probe[0]) - 100])
    bridges = [build_bridge(sess, ops, [build], [0], RICH_BOUT) for _ in range(3)]
    try:
        T = tg_types(ops, probe)
        plain = ops.lookup_join(sess, bridges[0], T, [0], RICH_POUT, join_type=join_type)
        try:
            for p in pages:
                plain.add_input(make_page(ops, p))
            ref = plain.drain()
        finally:
            plain.close()
        assert sum(len(p[0]["values"]) for p in ref) > len(probe[0]) // 2
        outs = []
        for bridge, prog in zip(bridges[1:], (TRUE, None)):
            _same_pages(run_probe(sess, ops, bridge, pages, [0], RICH_POUT, join_type,
                                  prog), ref)
        if join_type >= 2:
            un = ref_unmatched(keys_of(build, [0]), keys_of(probe, [0]))
            for bridge in bridges:
                outs.append(emit_outer(sess, ops, bridge, build, RICH_BOUT,
                                       [probe[ch] for ch in RICH_POUT], un))
    finally:
        for b in bridges:
            b.close()


@pytest.mark.parametrize("join_type", ALL_TYPES, ids=JT_IDS)
def test_constant_false(sess, ops, join_type):
    """inner: zero rows per page; LEFT: every probe row NULL-extended;
    RIGHT / FULL: the lookup-outer operator emits every build row"""
    build, probe = rich_tables(seed=9)
    pages = split_pages(probe, [100, 0, len(probe[0]) - 100])
    un, refs = filtered_case(sess, ops, [build], [0], RICH_BOUT, [pages], [0],
                             RICH_POUT, join_type, [FALSE], cover=False)
    eop, eob = refs[0]
    if join_type in (1, 3):
        assert np.array_equal(eop, np.arange(len(probe[0]))) and (eob == -1).all()
    else:
        assert len(eop) == 0
    assert np.array_equal(un, np.arange(len(build[0])))


# --------------------------------------------------------------------------
# join shapes
# --------------------------------------------------------------------------
@pytest.mark.parametrize("join_type", ALL_TYPES, ids=JT_IDS)
def test_multi_page_build_and_probe(sess, ops, join_type):
    build, probe = rich_tables(seed=12, nb=1000, m=600)
    bpages = split_pages(build, [37, 64, 0, 1, 100, 798])
    ppages = split_pages(probe, [65, 0, 1, 200, 334])
    filtered_case(sess, ops, bpages, [0], RICH_BOUT, [ppages], [0], RICH_POUT,
                  join_type, [RICH_FILTERS["ne_q21"]])


@pytest.mark.parametrize("join_type", ALL_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("name", ["bigint_integer", "varchar_bigint", "double"])
def test_generic_keys_fixed_width_filter(sess, ops, name, join_type):
    """multi-channel, VARCHAR and DOUBLE keys; the filter reads two appended
    BIGINT channels (the VARCHAR key channels stay unnamed)"""
    build, bk, probe, pk = generic_tables(name)
    r = rng(21)
    nb, m = len(build[0]), len(probe[0])
    build.insert(len(bk), nullable("i64", r.integers(0, 3, nb), r.random(nb) < 0.1, POISON_I))
    probe.insert(len(pk), nullable("i64", r.integers(0, 3, m), r.random(m) < 0.1, POISON_I))
    nk = len(pk)
    prog = (C(nk), C(len(probe) + nk), "ne")
    filtered_case(sess, ops, [build], bk, list(range(len(build))), [[probe]], pk,
                  list(range(len(probe))), join_type, [prog])


@pytest.mark.parametrize("join_type", [2, 3], ids=["right", "full"])
def test_two_filters_share_a_bridge(sess, ops, join_type):
    """two recording operators with different filters: the visited set is
    the union of their surviving pairs"""
    build, probe = rich_tables(seed=14)
    a, b = RICH_FILTERS["ne_q21"], RICH_FILTERS["between"]
    un, _ = filtered_case(sess, ops, [build], [0], RICH_BOUT, [[probe], [probe]], [0],
                          RICH_POUT, join_type, [a, b])
    rows = [py_reference(build, probe, [0], [0], p, False, False)[2] for p in (a, b)]
    assert np.array_equal(un, np.intersect1d(*rows))
    assert len(un) < min(len(rows[0]), len(rows[1]))    # each adds to the other


@pytest.mark.parametrize("join_type", ALL_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("shape", ["empty_build", "all_null_probe"])
def test_empty_sides(sess, ops, shape, join_type):
    build, probe = rich_tables(seed=15)
    if shape == "empty_build":
        build = [c.slice(0, 0, False) for c in build]
    else:
        probe[0] = Col("i64", probe[0].values, np.zeros(len(probe[0]), bool))
    _, refs = filtered_case(sess, ops, [build], [0], RICH_BOUT, [[probe]], [0],
                            RICH_POUT, join_type, [RICH_FILTERS["ne_q21"]], cover=False)
    assert len(refs[0][0]) == (len(probe[0]) if join_type in (1, 3) else 0)


# --------------------------------------------------------------------------
# sizes: single BIGINT key, filter probe.x <> build.y, vectorised reference
# --------------------------------------------------------------------------
NE = (C(1), C(3 + 1), "ne")


def ne_pred(build, probe):
    x, xv, y, yv = probe[1].values, probe[1].valid, build[1].values, build[1].valid

    def pred(op, ob):
        ok = xv[op] & yv[ob]
        return ok & (x[op] != y[ob]), ~ok
    return pred


def sized_tables(n_cand, m, seed=0):
    """exactly n_cand candidate pairs over m probe rows. With six or more
    candidates: key A on three build rows (y = pass, fail, NULL), key B on
    two (both fail), key C on one, every further candidate a unique key; the
    hitting probe rows sit at random places among misses and NULL keys."""
    r = rng(seed + n_cand + m)
    groups = 3 if n_cand >= 6 else 0
    uniq = n_cand - 6 if groups else n_cand
    hits = groups + uniq
    assert m >= hits
    g = np.concatenate([[0, 0, 0, 1, 1, 2][:6 if groups else 0],
                        3 + np.arange(uniq)]).astype(np.int64)
    nb = len(g)
    y = r.integers(0, 3, nb)
    ynull = r.random(nb) < 0.1
    perm = r.permutation(nb)
    place = np.sort(r.choice(m, hits, replace=False))
    pg = np.full(m, -1, np.int64)
    pg[place] = np.concatenate([np.arange(groups), 3 + np.arange(uniq)])
    x = r.integers(0, 3, m)
    xnull = r.random(m) < 0.1
    if groups:
        y[:6] = [1, 0, 2, 0, 0, 1]
        ynull[:6] = [False, False, True, False, False, False]
        x[place[:3]] = 0
        xnull[place[:3]] = False
    pk = np.where(pg >= 0, key_of(np.maximum(pg, 0)), key_of(10 * (nb + 1) + np.arange(m)))
    pnull = (pg < 0) & (np.arange(m) % 5 == 0)
    brow = np.empty(nb, np.int64)
    brow[perm] = np.arange(nb)                   # group row k sits at build row brow[k]
    bk, by, bnull = np.empty(nb, np.int64), np.empty(nb, np.int64), np.empty(nb, bool)
    bk[brow], by[brow], bnull[brow] = key_of(g), y, ynull
    build = [Col("i64", bk), nullable("i64", by, bnull, POISON_I),
             Col("i64", np.arange(nb))]
    probe = [nullable("i64", pk, pnull), nullable("i64", x, xnull, POISON_I),
             Col("i64", np.arange(m))]
    op, _ = ref_join_vec(bk, None, pk, ~pnull)
    assert len(op) == n_cand
    return build, probe


def sized_case(sess, ops, n_cand, m, join_type, **kw):
    build, probe = sized_tables(n_cand, m)
    return filtered_case(sess, ops, [build], [0], [0, 1, 2], [[probe]], [0], [0, 1, 2],
                         join_type, [NE], preds=[ne_pred(build, probe)],
                         cover=n_cand >= 6, **kw)


SCAN_EDGES = (JSCAN_CHUNK - 1, JSCAN_CHUNK, JSCAN_CHUNK + 1, 2 * JSCAN_CHUNK + 1)
GRID_STRIDE_N = GRID_THREADS + 197


@pytest.mark.parametrize("join_type", ALL_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("n_cand", [0, 1, 63, 64, 65, 257])
def test_candidate_count_wave_edges(sess, ops, n_cand, join_type):
    sized_case(sess, ops, n_cand, n_cand + 40, join_type)


@pytest.mark.parametrize("join_type", [0, 3], ids=["inner", "full"])
@pytest.mark.parametrize("n_cand", SCAN_EDGES)
def test_candidate_count_scan_chunk_edges(sess, ops, n_cand, join_type):
    """run_scan_counts over the keep flags: JSCAN_CHUNK candidates"""
    sized_case(sess, ops, n_cand, n_cand + 100, join_type)


@pytest.mark.parametrize("join_type", [1, 3], ids=["left", "full"])
@pytest.mark.parametrize("m", SCAN_EDGES)
def test_probe_row_scan_chunk_edges(sess, ops, m, join_type):
    """run_scan_counts over the survivor counts and the survivor-less flags:
    JSCAN_CHUNK probe rows, a third of them with a candidate"""
    sized_case(sess, ops, m // 3, m, join_type)


@pytest.mark.parametrize("join_type", ALL_TYPES, ids=JT_IDS)
def test_grid_stride(sess, ops, join_type):
    """the second stride of every per-pair and per-probe-row kernel"""
    sized_case(sess, ops, GRID_STRIDE_N, GRID_STRIDE_N + 1000, join_type)


# --------------------------------------------------------------------------
# hot probe rows: 1000 candidates each, crossing waves and a block
# --------------------------------------------------------------------------
HOT = 1000
HOT_FILTERS = {          # (build channel, constant): build.ch == constant
    "every_third": (1, 0), "none": (1, 7), "first_only": (2, 0), "last_only": (2, HOT - 1)}


def hot_tables(n_hot_rows, ch, target):
    """build [key, third, pos, row]: HOT rows of one key (third = copy % 3,
    pos = place in the descending emission order), then the coverage groups
    A (target, other, NULL in channel `ch`) and B (other, other), then unique
    keys; probe [key, row]: a miss, A, n_hot_rows x the hot key, B, misses"""
    r = rng(n_hot_rows)
    nb = HOT + 5 + 50
    g = np.concatenate([np.zeros(HOT), [1, 1, 1, 2, 2], 3 + np.arange(50)]).astype(np.int64)
    third = np.concatenate([np.arange(HOT) % 3, [3] * 5, np.full(50, 3)]).astype(np.int64)
    pos = np.full(nb, HOT + 5, np.int64)
    tnull = np.zeros(nb, bool)
    vals = [third, pos][ch - 1]
    vals[HOT:HOT + 5] = [target, target + 1, target, target + 1, target + 1]
    tnull[HOT + 2] = True
    perm = r.permutation(nb)
    brow = np.empty(nb, np.int64)
    brow[perm] = np.arange(nb)
    hot_rows = np.sort(brow[:HOT])[::-1]         # emission order: descending row
    pos_at = pos.copy()
    bk, b3, bp, bn = (np.empty(nb, np.int64) for _ in range(4))
    bk[brow], b3[brow], bp[brow], bn[brow] = key_of(g), third, pos_at, tnull
    bp[hot_rows] = np.arange(HOT)
    nulls = [bn.astype(bool) if ch == 1 else np.zeros(nb, bool),
             bn.astype(bool) if ch == 2 else np.zeros(nb, bool)]
    build = [Col("i64", bk), nullable("i64", b3, nulls[0], POISON_I),
             nullable("i64", bp, nulls[1], POISON_I), Col("i64", np.arange(nb))]
    pg = np.concatenate([[-1, 1], np.zeros(n_hot_rows), [2, -1, 5, -1]]).astype(np.int64)
    pk = np.where(pg >= 0, key_of(np.maximum(pg, 0)), key_of(1000 + np.arange(len(pg))))
    probe = [Col("i64", pk), Col("i64", np.arange(len(pk)))]
    return build, probe


@pytest.mark.parametrize("join_type", ALL_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("n_hot_rows", [1, 64])
@pytest.mark.parametrize("name", list(HOT_FILTERS))
def test_hot_probe_rows(sess, ops, name, n_hot_rows, join_type):
    ch, target = HOT_FILTERS[name]
    build, probe = hot_tables(n_hot_rows, ch, target)
    prog = (C(2 + ch), I(target), "eq")
    v, vv = build[ch].values, build[ch].valid

    def pred(op, ob):
        return vv[ob] & (v[ob] == target), ~vv[ob]
    _, refs = filtered_case(sess, ops, [build], [0], [0, 1, 2, 3], [[probe]], [0], [0, 1],
                            join_type, [prog], preds=[pred])
    eop, eob = refs[0]
    per_hot = {"every_third": (HOT + 2) // 3, "none": 0, "first_only": 1,
               "last_only": 1}[name]
    hot = (eop >= 2) & (eop < 2 + n_hot_rows) & (eob >= 0)
    assert hot.sum() == per_hot * n_hot_rows


# --------------------------------------------------------------------------
# partitioned probe (inner and right), and its overflow retry
# --------------------------------------------------------------------------
@pytest.mark.parametrize("join_type", [0, 2], ids=["inner", "right"])
@pytest.mark.parametrize("n_cand", [65, 1000])
def test_partitioned_probe(sess, ops, partitioned, n_cand, join_type):
    sized_case(sess, ops, n_cand, n_cand + 40, join_type, order="list")


@pytest.mark.parametrize("join_type", [0, 2], ids=["inner", "right"])
def test_partitioned_probe_overflow_retry(sess, ops, partitioned, join_type):
    """64 x 64 candidates of one key against the first-try cap, filtered by
    probe.x <> build.y"""
    r = rng(6)
    n = OVERFLOW_N
    k = key_of(np.full(n, 5))
    build = [Col("i64", k), nullable("i64", r.integers(0, 3, n), r.random(n) < 0.1, POISON_I),
             Col("i64", np.arange(n))]
    probe = [Col("i64", k.copy()), nullable("i64", r.integers(0, 4, n), r.random(n) < 0.1,
                                            POISON_I), Col("i64", np.arange(n))]
    probe[1].values[7] = 3                       # loses only the NULL pairs ...
    probe[1].valid[7] = True
    probe[1].valid[9] = False                    # ... and one that loses everybody
    _, refs = filtered_case(sess, ops, [build], [0], [0, 1, 2], [[probe]], [0], [0, 1, 2],
                            join_type, [NE], preds=[ne_pred(build, probe)], order="list")
    assert 0 < len(refs[0][0]) < n * n


def test_partitioned_left_takes_classic_path(sess, ops, partitioned):
    sized_case(sess, ops, 257, 300, 1)


# --------------------------------------------------------------------------
# the Q21 shape: lineitem self-join LEFT on orderkey, l2.suppkey <> l1.suppkey
# --------------------------------------------------------------------------
def test_q21_shape(sess, ops):
    r = rng(21)
    n = 3000
    okey = np.sort(r.integers(0, n // 4, n)).astype(np.int64)
    supp = r.integers(0, 5, n).astype(np.int64)
    rows = np.arange(n, dtype=np.int64)
    l1 = [Col("i64", okey), Col("i64", supp), Col("i64", rows)]
    prog = (C(1), C(3 + 1), "ne")
    build_cols = l1
    bridge = build_bridge(sess, ops, [l1], [0], [0, 1, 2])
    try:
        pages = run_probe(sess, ops, bridge, [l1], [0], [0, 1, 2], 1, prog)
    finally:
        bridge.close()
    got = output_cols(ops, pages, 6)
    # plain Python: per l1 row, the l2 rows of its order with another supplier
    by_order = {}
    for i in range(n):
        by_order.setdefault(int(okey[i]), []).append(i)
    want = [sum(1 for j in by_order[int(okey[i])] if supp[j] != supp[i]) for i in range(n)]
    assert 0 in want and max(want) >= 2
    surv = np.bincount(got[2].values[got[5].valid], minlength=n)
    assert surv.tolist() == want
    lone = np.bincount(got[2].values[~got[5].valid], minlength=n)
    assert lone.tolist() == [1 if w == 0 else 0 for w in want]
    assert np.array_equal(got[2].values, np.sort(got[2].values))
    ok = got[5].valid
    assert (got[1].values[ok] != got[4].values[ok]).all()
    assert (got[0].values[ok] == got[3].values[ok]).all()
    eop, eob, _ = py_reference(build_cols, l1, [0], [0], prog, True, False)
    check_inner(ops, pages, [l1], [0], [0, 1, 2], build_cols, [0], [0, 1, 2], True,
                ORDER, (eop, eob))


# --------------------------------------------------------------------------
# errors: the status, and nothing launched (the operator stays usable or
# was never made)
# --------------------------------------------------------------------------
def expect_error(fn, status, *words):
    import trino_amd
    with pytest.raises(trino_amd.TrinoGpuError) as ei:
        fn()
    msg = str(ei.value)
    assert msg.startswith(f"status {status}:"), msg
    for w in words:
        assert w in msg, msg


@pytest.fixture
def err_bridge(sess, ops):
    build = [Col("i64", np.arange(20)), Col("str", [b"s%d" % i for i in range(20)]),
             Col("i64", np.arange(20))]
    bridge = build_bridge(sess, ops, [build], [0], [0, 2])
    yield bridge
    bridge.close()


def _err_probe():
    return [Col("i64", np.arange(10)), Col("str", [b"p"] * 10), Col("i64", np.arange(10))]


@pytest.mark.parametrize("prog,status,word", [
    ((C(2), C(3 + 1), "ne"), TG_ERR_UNSUPPORTED, "VARCHAR"),       # build VARCHAR
    ((C(1), C(3 + 2), "ne"), TG_ERR_UNSUPPORTED, "VARCHAR"),       # probe VARCHAR
    ((C(2), C(3 + 3), "ne"), TG_ERR_INVALID_ARG, "column index"),  # past the build
    ((C(2), C(1000), "ne"), TG_ERR_INVALID_ARG, "column index"),
], ids=["varchar_build", "varchar_probe", "index_one_past", "index_far"])
def test_add_input_errors(sess, ops, err_bridge, prog, status, word):
    probe = _err_probe()
    op = ops.lookup_join(sess, err_bridge, tg_types(ops, probe), [0], [0, 2],
                         join_type=1, filter=ops.expr(*prog))
    try:
        page = make_page(ops, probe)
        expect_error(lambda: op.add_input(page), status, word)
        expect_error(lambda: op.add_input(page), status, word)    # and again
        assert op.drain() == []
    finally:
        op.close()


def test_create_errors(sess, ops, err_bridge):
    T = tg_types(ops, _err_probe())

    def create(prog, join_type=0):
        e = prog if not isinstance(prog, tuple) else ops.expr(*prog)
        return lambda: ops.lookup_join(sess, err_bridge, T, [0], [0, 2],
                                       join_type=join_type, filter=e)
    deep = tuple(C(0) for _ in range(MAX_STACK + 1)) + ("add",) * MAX_STACK
    expect_error(create(deep), TG_ERR_INVALID_ARG, "depth")
    ok = tuple(C(0) for _ in range(MAX_STACK)) + ("add",) * (MAX_STACK - 1)
    ops.lookup_join(sess, err_bridge, T, [0], [0, 2], filter=ops.expr(*ok)).close()
    expect_error(create((C(0), C(2))), TG_ERR_INVALID_ARG, "one value")
    expect_error(create((C(0), "add")), TG_ERR_INVALID_ARG, "underflow")
    raw = ops.expr(C(0), I(1), "eq")
    raw.insts[2].op = 17
    expect_error(create(raw), TG_ERR_UNSUPPORTED, "opcode")
    expect_error(create((C(0), C(3), "ne"), join_type=4), TG_ERR_INVALID_ARG, "join_type")
    # a rejected join_type 2 | 3 creation is not counted as a recording operator
    expect_error(create(deep, join_type=2), TG_ERR_INVALID_ARG, "depth")
    out = ops.lookup_outer(sess, err_bridge, [ops.TG_BIGINT])
    try:
        assert len(out.drain()) == 1
    finally:
        out.close()


def test_set_builder_bridge(sess, ops):
    build = [Col("i64", np.arange(100))]          # dense range: the bitmap
    bridge = build_bridge(sess, ops, [build], [0], [], set_builder=True)
    probe = [Col("i64", np.arange(10)), Col("i64", np.arange(10))]
    op = ops.lookup_join(sess, bridge, tg_types(ops, probe), [0], [0, 1],
                         filter=ops.expr(C(1), C(2), "ne"))
    try:
        page = make_page(ops, probe)
        expect_error(lambda: op.add_input(page), TG_ERR_UNSUPPORTED, "set-builder")
    finally:
        op.close()
        bridge.close()
