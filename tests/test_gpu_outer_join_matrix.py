"""RIGHT / FULL outer join parity matrix: lookup join with join_type 2
(build-outer) and 3 (full) plus the lookup-outer operator, against the exact
references of tests/test_gpu_join_matrix.py (ref_join, ref_join_vec) and
tests/test_outer_join_reference.py (ref_unmatched, ref_unmatched_vec).

Contract checked, bit-exactly and in list order, no tolerances:
 - the probe operator's output under join_type 2 | 3 is what ref_join gives
   with outer False | True (and is byte-identical to join_type 0 | 1);
 - after every recording probe operator on the bridge has finished, the
   lookup-outer operator emits ONE page holding exactly ref_unmatched's build
   rows, ascending: the probe output columns all NULL (cleared validity bit,
   zero-length VARCHAR), the build output columns gathered from the build
   row, their own NULLs kept; no page when nothing is unmatched.
Under TG_JOIN_CSR=0 the pairs of one probe row compare as a set, as in the
join matrix; the unmatched rows are ascending in every variant.

Every page carries its global row number as the last BIGINT column, and NULL
cells sit over poison words exactly as in the join matrix (a NULL build key
over a key the probe asks for is still emitted as unmatched).

Sizes are the smallest at which each path can go wrong: the bitmap word
edges (63 | 64 | 65 ...), more than GRID_THREADS matches for the second
stride of k_mark_visited, and JSCAN_CHUNK bitmap words (= JSCAN_CHUNK * 64
build rows) for the chunk edge of run_scan_counts, which the emission runs
over its per-word counts.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_join_matrix import (  # noqa: F401  (sess, ops, partitioned: fixtures)
    BIG_BUILD, CORE_CASES, GENERIC, GRID_STRIDE_M, GRID_THREADS, JSCAN_CHUNK,
    MULTI_PAGE_SIZES, ORDER, OVERFLOW_N, POISON_I, POISON_S, SHAPES, SMALL_M, Col,
    assert_col_equal, big_inputs, big_reference, bigint_tables, build_bridge,
    concat_cols, generic_tables, key_of, keys_of, make_page, nullable, ops,
    outer_column_tables, output_cols, overflow_inputs, partitioned, ref_join,
    ref_join_vec, rng, sess, source_constants, split_pages, tg_types)
from test_outer_join_reference import ref_unmatched, ref_unmatched_vec

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TG_ERR_INVALID_ARG, TG_ERR_STATE, TG_ERR_UNSUPPORTED = 1, 4, 6
JOIN_TYPES = [2, 3]
JT_IDS = ["right", "full"]
WORD = 64                                    # build rows per visited-bitmap word
WORD_EDGE_BUILDS = (0, 1, 63, 64, 65, 127, 128, 129, 1000)


# --------------------------------------------------------------------------
# runner
# --------------------------------------------------------------------------
def check_inner(ops, pages, probe_pages, pkeys, pout, build_cols, bkeys, bout,
                outer, order, pairs=None):
    """the probe operator's pages against ref_join (probe_join's comparison)"""
    probe_cols = concat_cols(probe_pages)
    assert len(pages) == len(probe_pages)        # one output page per input page
    if pairs is None:
        ref = ref_join(keys_of(build_cols, bkeys), keys_of(probe_cols, pkeys), outer)
        eop = np.array([p for p, _ in ref], np.int64)
        eob = np.array([-1 if b is None else b for _, b in ref], np.int64)
    else:
        eop, eob = pairs
    got = output_cols(ops, pages, len(pout) + len(bout))
    assert len(got[0]) == len(eop), f"output rows {len(got[0])} != {len(eop)}"
    if order == "set":          # TG_JOIN_CSR=0: pairs of a probe row as a set
        gop = got[len(pout) - 1].values
        gob = np.where(got[-1].valid, got[-1].values, -1)
        assert np.array_equal(gop, eop)
        gperm, eperm = np.lexsort((gob, gop)), np.lexsort((eob, eop))
        got = [Col(c.kind, [c.values[i] for i in gperm] if c.kind == "str"
                   else c.values[gperm], c.valid[gperm]) for c in got]
        eop, eob = eop[eperm], eob[eperm]
    for j, ch in enumerate(pout):
        assert_col_equal(got[j], probe_cols[ch], eop, f"probe channel {ch}")
    for j, ch in enumerate(bout):
        assert_col_equal(got[len(pout) + j], build_cols[ch], eob, f"build channel {ch}")
    return got


def probe_recording(sess, ops, bridge, probe_pages, pkeys, pout, join_type):
    """all pages through one recording operator, finished and closed"""
    op = ops.lookup_join(sess, bridge, tg_types(ops, probe_pages[0]), pkeys, pout,
                         join_type=join_type)
    try:
        for p in probe_pages:
            op.add_input(make_page(ops, p))
        return op.drain()
    finally:
        op.close()


def emit_outer(sess, ops, bridge, build_cols, bout, pout_cols, unmatched):
    """drain a lookup-outer operator and check its page against `unmatched`
    (ascending global build rows); pout_cols give the probe output kinds"""
    unmatched = np.asarray(unmatched, np.int64)
    op = ops.lookup_outer(sess, bridge, tg_types(ops, pout_cols))
    try:
        pages = op.drain()
    finally:
        op.close()
    if len(unmatched) == 0:
        assert pages == [], "a page although no build row is unmatched"
        return None
    assert len(pages) == 1, f"{len(pages)} pages from the lookup-outer operator"
    got = output_cols(ops, pages, len(pout_cols) + len(bout))
    assert len(got[0]) == len(unmatched), \
        f"unmatched rows {len(got[0])} != {len(unmatched)}"
    for j, c in enumerate(pout_cols):            # the all-NULL probe side
        assert got[j].kind == c.kind, f"probe output {j}: kind"
        assert not got[j].valid.any(), f"probe output {j}: a cell is not NULL"
    for j, ch in enumerate(bout):
        assert_col_equal(got[len(pout_cols) + j], build_cols[ch], unmatched,
                         f"unmatched build channel {ch}")
    assert got[-1].valid.all() and np.array_equal(got[-1].values, unmatched)
    return got


def outer_case(sess, ops, build_pages, bkeys, bout, probes, pkeys, pout,
               join_type, order=ORDER, pairs=None, unmatched=None):
    """build, then one recording operator per entry of `probes` (each a
    non-empty list of pages), each checked against ref_join, then the
    lookup-outer operator against ref_unmatched over all probe rows"""
    build_cols = concat_cols(build_pages)
    bridge = build_bridge(sess, ops, build_pages, bkeys, bout)
    try:
        for i, probe_pages in enumerate(probes):
            pages = probe_recording(sess, ops, bridge, probe_pages, pkeys, pout,
                                    join_type)
            check_inner(ops, pages, probe_pages, pkeys, pout, build_cols, bkeys,
                        bout, join_type == 3, order,
                        None if pairs is None else pairs[i])
        if unmatched is None:
            every = concat_cols([p for pp in probes for p in pp])
            unmatched = ref_unmatched(keys_of(build_cols, bkeys),
                                      keys_of(every, pkeys))
        pout_cols = [probes[0][0][ch] for ch in pout]
        return emit_outer(sess, ops, bridge, build_cols, bout, pout_cols, unmatched)
    finally:
        bridge.close()


def single_key_outer(sess, ops, shape, nb, m, join_type, **kw):
    build, probe = bigint_tables(*SHAPES[shape](nb, m, seed=nb + m))
    return outer_case(sess, ops, [build], [0], [0, 1, 2], [[probe]], [0], [0, 1],
                      join_type, **kw)


def status_of(ei):
    return int(str(ei.value).split(":")[0].split()[1])


# --------------------------------------------------------------------------
# 1. core: also under TG_JOIN_KV=1 and TG_JOIN_CSR=0 in child processes
# --------------------------------------------------------------------------
@pytest.mark.parametrize("join_type", JOIN_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("shape,nb", CORE_CASES)
def test_core_outer(sess, ops, shape, nb, join_type):
    got = single_key_outer(sess, ops, shape, nb, SMALL_M, join_type)
    assert got is not None                       # half the probe misses


def _run_child(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x",
           "-k", "test_core", "-p", "no:cacheprovider"]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, **env), cwd=_ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
    except subprocess.TimeoutExpired:
        pytest.exit(f"outer join matrix child {env} hit its time limit: nothing "
                    "more is started on the GPU", returncode=3)
    if r.returncode < 0 or r.returncode >= 128:
        pytest.exit(f"outer join matrix child {env} ended on a signal "
                    f"(status {r.returncode}): nothing more is started on the "
                    f"GPU\n{r.stdout[-3000:]}", returncode=3)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:]


def test_variant_kv_table():
    """core subset under TG_JOIN_KV=1: full list-order contract"""
    _run_child({"TG_JOIN_KV": "1"})


def test_variant_legacy_table():
    """core subset under TG_JOIN_CSR=0: pairs of each probe row as a set, the
    unmatched rows still ascending"""
    _run_child({"TG_JOIN_CSR": "0"})


# --------------------------------------------------------------------------
# 2. bitmap word edges
# --------------------------------------------------------------------------
def word_edge_tables(nb, pattern):
    """unique build keys; the probe hits exactly the rows `pattern` leaves
    matched and adds misses"""
    r = rng(1000 + nb)
    bk = key_of(r.permutation(nb))
    miss = key_of(10 * nb + 7 + np.arange(5))
    pnull = None
    if pattern == "all_miss":
        pk = key_of(10 * nb + 7 + np.arange(SMALL_M))
    elif pattern == "all_null_probe":
        pk = r.choice(bk, SMALL_M) if nb else key_of(np.arange(SMALL_M))
        pnull = np.ones(SMALL_M, bool)
    else:
        hit = np.ones(nb, bool)
        if pattern == "first_unmatched":
            hit[:1] = False
        elif pattern == "last_unmatched":
            hit[nb - 1:] = False
        elif pattern == "every_other":
            hit[0::2] = False
        else:
            assert pattern == "all_matched"
        pk = r.permutation(np.concatenate([bk[hit], miss]))
    return bigint_tables(bk, None, pk, pnull)


@pytest.mark.parametrize("join_type", JOIN_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("pattern", ["all_matched", "all_miss", "all_null_probe",
                                     "first_unmatched", "last_unmatched",
                                     "every_other"])
@pytest.mark.parametrize("nb", WORD_EDGE_BUILDS)
def test_bitmap_word_edges(sess, ops, nb, pattern, join_type):
    """builds of 0, 1, 63 | 64 | 65, 127 | 128 | 129 and 1000 rows: full and
    partial tail words of the visited bitmap (k_unvisited_count's mask)"""
    build, probe = word_edge_tables(nb, pattern)
    got = outer_case(sess, ops, [build], [0], [0, 1, 2], [[probe]], [0], [0, 1],
                     join_type)
    n_out = 0 if got is None else len(got[0])
    expect = {"all_matched": 0, "all_miss": nb, "all_null_probe": nb,
              "first_unmatched": min(nb, 1), "last_unmatched": min(nb, 1),
              "every_other": (nb + 1) // 2}[pattern]
    assert n_out == expect


# --------------------------------------------------------------------------
# 3. hot rows: the wave-combine and skip-if-set logic of k_mark_visited
# --------------------------------------------------------------------------
@pytest.mark.parametrize("join_type", JOIN_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("shape", ["one_hot", "dups"])
def test_hot_rows(sess, ops, shape, join_type):
    single_key_outer(sess, ops, shape, 1000, SMALL_M, join_type)


@pytest.mark.parametrize("join_type", JOIN_TYPES, ids=JT_IDS)
def test_every_probe_hits_the_hot_key(sess, ops, join_type):
    """500 copies of one key asked for by every probe row: 257 x 500 matches
    that all fall on the same 500 bits, page after page"""
    bk, _, _, _ = SHAPES["one_hot"](1000, SMALL_M, seed=3)
    pk = np.full(SMALL_M, key_of(0))
    build, probe = bigint_tables(bk, None, pk, None)
    probes = [split_pages(probe, [200, 57])]
    got = outer_case(sess, ops, [build], [0], [0, 1, 2], probes, [0], [0, 1],
                     join_type)
    assert len(got[0]) == 500


# --------------------------------------------------------------------------
# 4. grid stride of k_mark_visited: more matches than GRID_THREADS
# --------------------------------------------------------------------------
@pytest.mark.parametrize("join_type", JOIN_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("layout", ["scattered", "runs"])
def test_mark_grid_stride(sess, ops, layout, join_type):
    """a unique 1000-row build probed by GRID_STRIDE_M rows that all hit, so
    total > GRID_THREADS; rows with row % 7 == 3 are never asked for.
    `scattered` spreads each build row's ~600 hits over the page, `runs`
    makes them adjacent (whole waves on one bit)"""
    nb, m = 1000, GRID_STRIDE_M
    assert m > GRID_THREADS == (source_constants()["TG_BLOCK"]
                                * source_constants()["TG_MAX_BLOCKS"])
    r = rng(44)
    bk = key_of(r.permutation(nb))
    asked = np.flatnonzero(np.arange(nb) % 7 != 3)
    if layout == "scattered":
        rows = r.choice(asked, m)
    else:
        rows = asked[np.arange(m) * len(asked) // m]
    pk = bk[rows]
    build, probe = bigint_tables(bk, None, pk, None, payload_nulls=False)
    pairs = ref_join_vec(bk, None, pk, None)
    assert len(pairs[0]) == m
    got = outer_case(sess, ops, [build], [0], [0, 1, 2], [[probe]], [0], [0, 1],
                     join_type, order="list", pairs=[pairs],
                     unmatched=ref_unmatched_vec(bk, None, pk, None))
    assert np.array_equal(got[-1].values, np.flatnonzero(np.arange(nb) % 7 == 3))


# --------------------------------------------------------------------------
# 5. emission scan edges
# --------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, WORD + 1], ids=["one_chunk", "chunk_plus_65"])
def test_emission_scan_chunk_edge(sess, ops, extra):
    """the emission scans one count per bitmap word with run_scan_counts,
    whose chunk is JSCAN_CHUNK counts = JSCAN_CHUNK * 64 build rows: a build
    that fills exactly one chunk, and one that puts two words (one full, one
    of a single row) into a second chunk. The probe matches a thinned-out
    neighbourhood of the chunk edge and of the last row plus a sparse sample
    of all rows"""
    assert source_constants()["JSCAN_CHUNK"] == JSCAN_CHUNK
    edge = JSCAN_CHUNK * WORD
    nb = edge + extra
    r = rng(55)
    bk = key_of(np.arange(nb))
    near = np.concatenate([np.arange(edge - 300, min(edge + 300, nb)),
                           np.arange(nb - 70, nb), np.arange(0, 130)])
    near = near[near % 3 != 1]
    rows = np.unique(np.concatenate([near, r.integers(0, nb, 100000)]))
    pk = bk[r.permutation(rows)]
    brow = np.arange(nb, dtype=np.int64)
    build = [Col("i64", bk), Col("i64", brow)]
    probe = [Col("i64", pk), Col("i64", np.arange(len(pk), dtype=np.int64))]
    unmatched = ref_unmatched_vec(bk, None, pk, None)
    assert len(unmatched) == nb - len(rows)
    outer_case(sess, ops, [build], [0], [1], [[probe]], [0], [1], 2,
               order="list", pairs=[ref_join_vec(bk, None, pk, None)],
               unmatched=unmatched)


@pytest.mark.parametrize("path", ["classic", "partitioned"])
def test_big_build_multi_page(request, sess, ops, path):
    """the join matrix's 2^20-row build (duplicates, 3 % NULL keys) arriving
    in pages of 37, 64, 0, 1, 100, 8000 and the rest, so global row numbers
    cross page boundaries inside bitmap words; against the vectorised
    references, through the classic and the partitioned probe"""
    if path == "partitioned":
        request.getfixturevalue("partitioned")
    bk, bnull, pk, pnull = big_inputs()
    build, probe = bigint_tables(bk, bnull, pk, pnull, payload_nulls=False)
    sizes = MULTI_PAGE_SIZES + [BIG_BUILD - sum(MULTI_PAGE_SIZES)]
    outer_case(sess, ops, split_pages(build, sizes), [0], [0, 1, 2], [[probe]],
               [0], [0, 1], 2, order="list", pairs=[big_reference()],
               unmatched=ref_unmatched_vec(bk, ~bnull, pk, ~pnull))


# --------------------------------------------------------------------------
# 6. partitioned probe
# --------------------------------------------------------------------------
@pytest.mark.parametrize("shape,nb", [(s, nb) for s in ("unique", "dups", "nulls",
                                                        "all_miss")
                                      for nb in (65, 1000)])
def test_partitioned_right(sess, ops, partitioned, shape, nb):
    """join_type 2 is eligible for the partitioned probe: the mark runs over
    the list its stable sort leaves behind"""
    single_key_outer(sess, ops, shape, nb, SMALL_M, 2, order="list")


def test_partitioned_right_overflow_retry(sess, ops, partitioned):
    build, probe = bigint_tables(*overflow_inputs())
    got = outer_case(sess, ops, [build], [0], [0, 1, 2], [[probe]], [0], [0, 1], 2,
                     order="list")
    assert got is None                           # every build row matched


def test_partitioned_full_takes_classic_path(sess, ops, partitioned):
    """join_type 3 is probe-outer, which the partitioned probe does not
    serve: same answers through the classic path"""
    single_key_outer(sess, ops, "nulls", 1000, SMALL_M, 3)


# --------------------------------------------------------------------------
# 7. generic and VARCHAR keys
# --------------------------------------------------------------------------
@pytest.mark.parametrize("join_type", JOIN_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("name", GENERIC)
def test_generic_keys(sess, ops, name, join_type):
    build, bk, probe, pk = generic_tables(name)
    bkeys = keys_of(build, bk)
    never = [i for i, k in enumerate(bkeys)
             if any(c is None or c != c for c in k)]
    got = outer_case(sess, ops, [build], bk, list(range(len(build))), [[probe]],
                     pk, list(range(len(probe))), join_type)
    # NULL-component and NaN build rows can never match: all are emitted
    assert set(never) <= set(got[-1].values.tolist())
    if name in ("double", "bigint_integer", "varchar_bigint", "integer"):
        assert never


# --------------------------------------------------------------------------
# 8. columns
# --------------------------------------------------------------------------
@pytest.mark.parametrize("join_type", JOIN_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("source_nulls", [False, True], ids=["dense", "nulls"])
def test_columns_every_width(sess, ops, source_nulls, join_type):
    """probe output columns of 8, 4, 2 and 1 bytes and VARCHAR on the all-NULL
    side; build output columns of every width and VARCHAR keep their own
    NULLs (over poison) and their bytes"""
    build, probe = outer_column_tables(source_nulls)
    m = len(probe[0])
    i = np.arange(m)
    probe = [probe[0], Col("f64", i * 0.25), nullable("i32", i * 3, i % 5 == 0, 2 ** 30),
             Col("date", 8000 + i), Col("i16", i - 100), Col("i8", i % 90),
             nullable("str", [b"p%d" % k * (k % 3) for k in range(m)], i % 7 == 2,
                      POISON_S),
             probe[1]]
    allb, allp = list(range(len(build))), list(range(len(probe)))
    got = outer_case(sess, ops, [build], [0], allb, [[probe]], [0], allp, join_type)
    assert got is not None and 0 < len(got[0]) < len(build[0])
    if source_nulls:
        assert any(not c.valid.all() for c in got[len(allp) + 1:-1])


def test_varchar_build_column_byte_exact(sess, ops):
    build = [Col("i64", [1, 2, 2, 3, 4]),
             Col("str", [b"one", b"", b"deux\0", b"three", b"\xff\xfe"]),
             Col("i64", np.arange(5))]
    probe = [Col("i64", [2, 7]), Col("str", [b"x", b"y"]), Col("i64", np.arange(2))]
    got = outer_case(sess, ops, [build], [0], [1, 2], [[probe]], [0], [1, 2], 2)
    assert got[0].values == [b"", b"", b""] and not got[0].valid.any()
    assert got[2].values == [b"one", b"three", b"\xff\xfe"]
    assert got[3].values.tolist() == [0, 3, 4]


# --------------------------------------------------------------------------
# 9. sharing and state
# --------------------------------------------------------------------------
def _state_tables(nb=300):
    bk = key_of(rng(9).permutation(nb))
    build, _ = bigint_tables(bk, None, bk[:1], None)
    return bk, build


def _probe_of(pk):
    return [Col("i64", pk), Col("i64", np.arange(len(pk), dtype=np.int64))]


def _expect_status(fn, status):
    import trino_amd
    with pytest.raises(trino_amd.TrinoGpuError) as ei:
        fn()
    assert status_of(ei) == status, str(ei.value)


@pytest.mark.parametrize("join_type", JOIN_TYPES, ids=JT_IDS)
@pytest.mark.parametrize("end", ["finish", "close"])
def test_two_recording_operators_share_a_bridge(sess, ops, join_type, end):
    """disjoint hits give the union; get_output is TG_ERR_STATE until the
    second operator has finished (or was closed), then gives the right rows"""
    bk, build = _state_tables()
    pa, pb = _probe_of(bk[:100]), _probe_of(bk[200:])
    T = tg_types(ops, pa)
    bridge = build_bridge(sess, ops, [build], [0], [0, 1, 2])
    a = ops.lookup_join(sess, bridge, T, [0], [0, 1], join_type=join_type)
    b = ops.lookup_join(sess, bridge, T, [0], [0, 1], join_type=join_type)
    outer = ops.lookup_outer(sess, bridge, T)
    try:
        a.add_input(make_page(ops, pa))
        check_inner(ops, a.drain(), [pa], [0], [0, 1], build, [0], [0, 1, 2],
                    join_type == 3, ORDER)
        _expect_status(outer.get_output, TG_ERR_STATE)
        b.add_input(make_page(ops, pb))
        _expect_status(outer.get_output, TG_ERR_STATE)
        if end == "finish":
            b.finish()
        else:
            b.close()
        pages = outer.drain()
        assert len(pages) == 1
        got = output_cols(ops, pages, 5)
        assert np.array_equal(got[-1].values, np.arange(100, 200))
        assert outer.get_output() == (None, True)    # drained: nothing more
    finally:
        for op in (outer, a, b):
            op.close()
        bridge.close()
    # the same through the runner, against the reference
    outer_case(sess, ops, [build], [0], [0, 1, 2], [[pa], [pb]], [0], [0, 1],
               join_type)


@pytest.mark.parametrize("probe_ops", [0, 1])
def test_zero_probe_pages_emit_every_row(sess, ops, probe_ops):
    """no probe operator at all, or a recording one that saw no page"""
    bk, build = _state_tables(130)
    bridge = build_bridge(sess, ops, [build], [0], [0, 1, 2])
    try:
        if probe_ops:
            op = ops.lookup_join(sess, bridge, [ops.TG_BIGINT] * 2, [0], [0, 1],
                                 join_type=2)
            assert op.drain() == []
            op.close()
        got = emit_outer(sess, ops, bridge, build, [0, 1, 2], _probe_of(bk[:0]),
                         np.arange(130))
        assert len(got[0]) == 130
    finally:
        bridge.close()


@pytest.mark.parametrize("join_type", JOIN_TYPES, ids=JT_IDS)
def test_empty_build_emits_nothing(sess, ops, join_type):
    build, probe = bigint_tables(*SHAPES["nulls"](8, SMALL_M, seed=1))
    empty = [c.slice(0, 0, False) for c in build]
    assert outer_case(sess, ops, [empty], [0], [0, 1, 2], [[probe]], [0], [0, 1],
                      join_type) is None


def test_outer_operator_is_a_source(sess, ops):
    bk, build = _state_tables(10)
    bridge = build_bridge(sess, ops, [build], [0], [0, 1, 2])
    outer = ops.lookup_outer(sess, bridge, [ops.TG_BIGINT])
    try:
        assert ops._lib.tg_operator_needs_input(outer._h) == 0
        page = make_page(ops, _probe_of(bk[:3]))
        _expect_status(lambda: outer.add_input(page), TG_ERR_STATE)
    finally:
        outer.close()
        bridge.close()


def test_unbuilt_bridge_is_a_state_error(sess, ops):
    bridge = ops.JoinBridge(sess)
    outer = ops.lookup_outer(sess, bridge, [ops.TG_BIGINT])
    try:
        _expect_status(outer.get_output, TG_ERR_STATE)
    finally:
        outer.close()
        bridge.close()


def test_set_builder_bridge_is_unsupported(sess, ops):
    build = [Col("i64", np.arange(100))]          # dense range: the bitmap
    bridge = build_bridge(sess, ops, [build], [0], [], set_builder=True)
    outer = ops.lookup_outer(sess, bridge, [ops.TG_BIGINT])
    try:
        _expect_status(outer.get_output, TG_ERR_UNSUPPORTED)
    finally:
        outer.close()
        bridge.close()


@pytest.mark.parametrize("plain", [0, 1], ids=["after_inner", "after_left"])
def test_plain_probe_poisons_the_visited_set(sess, ops, plain):
    """after a join_type 0 or 1 operator probed the bridge its matches are
    unknown: TG_ERR_STATE, also when a recording operator probed as well"""
    bk, build = _state_tables(100)
    probe = _probe_of(bk[:40])
    T = tg_types(ops, probe)
    bridge = build_bridge(sess, ops, [build], [0], [0, 1, 2])
    outer = ops.lookup_outer(sess, bridge, T)
    try:
        probe_recording(sess, ops, bridge, [probe], [0], [0, 1], 2)
        op = ops.lookup_join(sess, bridge, T, [0], [0, 1], join_type=plain)
        op.add_input(make_page(ops, probe))
        op.drain()
        op.close()
        _expect_status(outer.get_output, TG_ERR_STATE)
    finally:
        outer.close()
        bridge.close()


@pytest.mark.parametrize("join_type", [4, -1])
def test_join_type_out_of_range(sess, ops, join_type):
    _, build = _state_tables(10)
    bridge = build_bridge(sess, ops, [build], [0], [0, 1, 2])
    try:
        _expect_status(lambda: ops.lookup_join(sess, bridge, [ops.TG_BIGINT] * 2, [0],
                                               [0, 1], join_type=join_type),
                       TG_ERR_INVALID_ARG)
        # the rejected creations were not counted as recording operators
        emit_outer(sess, ops, bridge, build, [0, 1, 2], [], np.arange(10))
    finally:
        bridge.close()


# --------------------------------------------------------------------------
# 10. join_type 2 == 0 and 3 == 1, byte for byte
# --------------------------------------------------------------------------
def _raw_pages(sess, ops, bridge, probe_pages, join_type):
    op = ops.lookup_join(sess, bridge, tg_types(ops, probe_pages[0]), [0], [0, 1],
                         join_type=join_type)
    try:
        for p in probe_pages:
            op.add_input(make_page(ops, p))
        return op.drain()
    finally:
        op.close()


@pytest.mark.parametrize("shape", ["dups", "colliding", "nulls"])
def test_inner_part_is_byte_identical(sess, ops, shape):
    """both operators of a pair probe the same built table, so their pages
    are compared raw, page by page: value bytes and validity bits"""
    build, probe = bigint_tables(*SHAPES[shape](1000, SMALL_M, seed=77))
    probe_pages = split_pages(probe, [100, 0, SMALL_M - 100])
    bridge = build_bridge(sess, ops, [build], [0], [0, 1, 2])
    try:
        for recording, plain in ((2, 0), (3, 1)):
            got = _raw_pages(sess, ops, bridge, probe_pages, recording)
            ref = _raw_pages(sess, ops, bridge, probe_pages, plain)
            assert len(got) == len(ref) == len(probe_pages)
            for gp, rp in zip(got, ref):
                assert len(gp) == len(rp) == 5
                for g, r in zip(gp, rp):
                    assert g["type"] == r["type"]
                    assert g["values"].tobytes() == r["values"].tobytes()
                    assert (g["valid"] is None) == (r["valid"] is None)
                    if g["valid"] is not None:     # the n bits the page owns
                        n = len(g["values"])
                        bits = [np.unpackbits(x["valid"].view(np.uint8),
                                              bitorder="little")[:n] for x in (g, r)]
                        assert np.array_equal(*bits)
    finally:
        bridge.close()


# --------------------------------------------------------------------------
# 11. randomised
# --------------------------------------------------------------------------
def _random_splits(r, n):
    cuts = np.sort(r.integers(0, n + 1, int(r.integers(0, 4))))
    return np.diff(np.concatenate([[0], cuts, [n]])).tolist()


def test_randomised_small_cases(sess, ops):
    """40 seeded cases: nb, m <= 300, key domain, NULL rate, page splits, one
    or two probe operators, join type 2 or 3, all against the references"""
    r = rng(2024)
    for case in range(40):
        nb, m = int(r.integers(0, 301)), int(r.integers(1, 301))
        dom = int(r.integers(1, 400))
        null_rate = float(r.choice([0.0, 0.05, 0.5]))
        bk = key_of(r.integers(0, dom, nb))
        pk = key_of(r.integers(0, dom + dom // 2 + 1, m))
        bnull, pnull = r.random(nb) < null_rate, r.random(m) < null_rate
        build, probe = bigint_tables(bk, bnull, pk, pnull)
        bpages = split_pages(build, _random_splits(r, nb))
        if r.integers(0, 2) and m >= 2:
            cut = int(r.integers(1, m))
            halves = [[Col("i64", pk[lo:hi], ~pnull[lo:hi]),
                       Col("i64", np.arange(hi - lo, dtype=np.int64))]
                      for lo, hi in ((0, cut), (cut, m))]
            probes = [split_pages(h, _random_splits(r, len(h[0]))) for h in halves]
        else:
            probes = [split_pages(probe, _random_splits(r, m))]
        join_type = int(r.choice(JOIN_TYPES))
        try:
            outer_case(sess, ops, bpages, [0], [0, 1, 2], probes, [0], [0, 1],
                       join_type)
        except AssertionError as e:
            raise AssertionError(f"case {case} (nb={nb}, m={m}, dom={dom}, "
                                 f"nulls={null_rate}, join_type={join_type}): {e}")
