"""References for the TopNRanking operator (TopNRankingOp in
trino_amd/csrc/ops_window.hip) and their own checks. No GPU.

ref_topn_ranking is the contract read literally: ref_window (the Window
operator's plain reference) with one ranking spec, restricted to the rows whose
ranking is <= N. ref_topn_ranking_vec is the same over ref_window_vec, for the
large shapes of tests/test_gpu_topn_ranking_matrix.py. independent_topn_ranking
shares no code with either: its own three-way cell comparison, partitions
collected in a dict, each partition a stably sorted list, rankings assigned
by explicit tie tests. Hand-written tables with typed-out outputs pin all of
them. The pruning argument of DESIGN.md §6i is run as an algorithm (cut
`retained + next page` again and again, then once more with the ranking), and
the rank cut's placement (per-chunk keep counts, a scan of the counts,
ballot-prefix positions) is modelled and compared with the list it must give.
"""
import functools
import math
import os
import re

import numpy as np
import pytest

from test_window_reference import (DENSE_RANK, RANGE, RANK, ROW_NUMBER, ref_window,
                                   ref_window_vec, source_constants, table_cols)

FNS = (ROW_NUMBER, RANK, DENSE_RANK)
FN_NAMES = ("row_number", "rank", "dense_rank")
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
NAN = math.nan

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------
# the reference: Window, then the cut
# --------------------------------------------------------------------------
def ref_topn_ranking(rows, part, sort, desc, fn, N, emit):
    """rows: tuples of cells (None = NULL). Returns (order, ranking): the
    kept rows as input row indices in output order, and their rankings (None
    without `emit`)."""
    order, (col,) = ref_window(rows, part, sort, desc, [(fn, -1, RANGE)])
    kept = [(i, r) for i, r in zip(order, col) if r <= N]
    return [i for i, _ in kept], [r for _, r in kept] if emit else None


def ref_topn_ranking_vec(cols, part, sort, desc, fn, N, emit):
    """the numpy twin: cols are Col objects; (order, ranking) as int64 arrays"""
    order, ((rank, _),) = ref_window_vec(cols, part, sort, desc, [(fn, -1, RANGE)])
    keep = rank <= N
    return order[keep], rank[keep] if emit else None


# --------------------------------------------------------------------------
# an independent reference
# --------------------------------------------------------------------------
def _cmp_asc(a, b):
    """three-way comparison under ASC: numbers (-0.0 == 0.0), then every NaN
    as one value, then NULL"""
    def cls(v):
        return 2 if v is None else 1 if isinstance(v, float) and v != v else 0
    ca, cb = cls(a), cls(b)
    if ca != cb:
        return -1 if ca < cb else 1
    if ca:
        return 0
    return -1 if a < b else 1 if a > b else 0


def _cmp_cells(x, y, desc):
    for a, b, d in zip(x, y, desc):
        c = _cmp_asc(a, b)
        if c:
            return -c if d else c       # DESC is ASC backwards, NULL first
    return 0


def independent_topn_ranking(rows, part, sort, desc, fn, N, emit):
    """per-partition sorted lists with explicit tie handling"""
    def canon(v):
        if v is None:
            return ("null",)
        if isinstance(v, float):
            return ("nan",) if v != v else ("num", v + 0.0)
        return ("num", v)

    partitions = {}                                    # canonical key -> row indices
    for i, row in enumerate(rows):
        partitions.setdefault(tuple(canon(row[c]) for c in part), []).append(i)
    pcells = lambda i: [rows[i][c] for c in part]      # noqa: E731
    scells = lambda i: [rows[i][c] for c in sort]      # noqa: E731
    heads = sorted((members[0] for members in partitions.values()),
                   key=functools.cmp_to_key(
                       lambda i, j: _cmp_cells(pcells(i), pcells(j), [0] * len(part))))
    order, ranking = [], []
    for h in heads:
        members = partitions[tuple(canon(rows[h][c]) for c in part)]
        members = sorted(members, key=functools.cmp_to_key(          # stable: ties keep input order
            lambda i, j: _cmp_cells(scells(i), scells(j), desc)))
        rank = dense = 0
        for pos, i in enumerate(members):
            tie = pos > 0 and _cmp_cells(scells(members[pos - 1]), scells(i), desc) == 0
            if not tie:
                rank = pos + 1
                dense += 1
            r = pos + 1 if fn == ROW_NUMBER else rank if fn == RANK else dense
            if r <= N:
                order.append(i)
                ranking.append(r)
    return order, ranking if emit else None


# --------------------------------------------------------------------------
# hand-written tables: (rows, part, sort, desc, N) -> per function (order, ranking)
# --------------------------------------------------------------------------
TABLES = {
    # the peer group (sort key 20) straddles N = 2: row_number cuts it, rank
    # keeps both peers, dense_rank keeps them as group 2
    "peer_group_straddles_n": dict(
        rows=[(1, 10), (1, 20), (1, 20), (1, 30), (2, 5), (2, 5), (2, 5)],
        part=[0], sort=[1], desc=[0], N=2,
        out={ROW_NUMBER: ([0, 1, 4, 5], [1, 2, 1, 2]),
             RANK: ([0, 1, 2, 4, 5, 6], [1, 2, 2, 1, 1, 1]),
             DENSE_RANK: ([0, 1, 2, 4, 5, 6], [1, 2, 2, 1, 1, 1])}),
    # rank skips: after two peers at 1 the next row has rank 3 > 2, dense_rank 2
    "rank_skips_dense_does_not": dict(
        rows=[(7,), (7,), (8,), (9,)], part=[], sort=[0], desc=[0], N=2,
        out={ROW_NUMBER: ([0, 1], [1, 2]),
             RANK: ([0, 1], [1, 1]),
             DENSE_RANK: ([0, 1, 2], [1, 1, 2])}),
    # DOUBLE sort key ASC: -0.0 ties with 0.0 (input order), NaN above +inf, NULL last
    "double_keys_asc": dict(
        rows=[(NAN,), (0.0,), (None,), (-0.0,), (math.inf,), (-NAN,)],
        part=[], sort=[0], desc=[0], N=3,
        out={ROW_NUMBER: ([1, 3, 4], [1, 2, 3]),
             RANK: ([1, 3, 4], [1, 1, 3]),
             DENSE_RANK: ([1, 3, 4, 0, 5], [1, 1, 2, 3, 3])}),
    # DESC: NULL first, then the NaNs as one value, then the numbers downwards
    "desc_null_first": dict(
        rows=[(3.0,), (None,), (NAN,), (5.0,), (None,)],
        part=[], sort=[0], desc=[1], N=2,
        out={ROW_NUMBER: ([1, 4], [1, 2]),
             RANK: ([1, 4], [1, 1]),
             DENSE_RANK: ([1, 4, 2], [1, 1, 2])}),
    # NULL is a partition value and its partition comes last
    "null_partition": dict(
        rows=[(None, 2), (4, 9), (None, 1), (4, 8), (None, 3)],
        part=[0], sort=[1], desc=[0], N=1,
        out={ROW_NUMBER: ([3, 2], [1, 1]),
             RANK: ([3, 2], [1, 1]),
             DENSE_RANK: ([3, 2], [1, 1])}),
    # no partition channel: one partition of everything
    "no_partition_channels": dict(
        rows=[(3,), (1,), (2,), (1,)], part=[], sort=[0], desc=[0], N=2,
        out={ROW_NUMBER: ([1, 3], [1, 2]),
             RANK: ([1, 3], [1, 1]),
             DENSE_RANK: ([1, 3, 2], [1, 1, 2])}),
    # no sort channel: every row of a partition is a peer; row_number keeps the
    # first N in input order, rank and dense_rank keep everything
    "no_sort_channels": dict(
        rows=[(2, 0), (1, 1), (2, 2), (1, 3), (2, 4)], part=[0], sort=[], desc=[], N=2,
        out={ROW_NUMBER: ([1, 3, 0, 2], [1, 2, 1, 2]),
             RANK: ([1, 3, 0, 2, 4], [1, 1, 1, 1, 1]),
             DENSE_RANK: ([1, 3, 0, 2, 4], [1, 1, 1, 1, 1])}),
    # neither: input order; row_number keeps the first N input rows
    "no_channels_at_all": dict(
        rows=[(4,), (None,), (-2,), (9,)], part=[], sort=[], desc=[], N=3,
        out={ROW_NUMBER: ([0, 1, 2], [1, 2, 3]),
             RANK: ([0, 1, 2, 3], [1, 1, 1, 1]),
             DENSE_RANK: ([0, 1, 2, 3], [1, 1, 1, 1])}),
    # N larger than every partition: everything, in the Window's order
    "n_above_every_partition": dict(
        rows=[(2, 5), (1, 7), (2, 4), (1, 7)], part=[0], sort=[1], desc=[1], N=100,
        out={ROW_NUMBER: ([1, 3, 0, 2], [1, 2, 1, 2]),
             RANK: ([1, 3, 0, 2], [1, 1, 1, 2]),
             DENSE_RANK: ([1, 3, 0, 2], [1, 1, 1, 2])}),
    # INT64 extremes as keys, DESC
    "int64_extremes_desc": dict(
        rows=[(I64_MIN,), (I64_MAX,), (0,), (I64_MAX,), (None,)],
        part=[], sort=[0], desc=[1], N=2,
        out={ROW_NUMBER: ([4, 1], [1, 2]),
             RANK: ([4, 1, 3], [1, 2, 2]),
             DENSE_RANK: ([4, 1, 3], [1, 2, 2])}),
}

REFS = {"window_then_cut": ref_topn_ranking, "independent": independent_topn_ranking}


@pytest.mark.parametrize("ref", sorted(REFS))
@pytest.mark.parametrize("name", sorted(TABLES))
def test_references_by_hand(name, ref):
    t = TABLES[name]
    assert len(t["rows"]) <= 8
    for fn in FNS:
        order, ranking = REFS[ref](t["rows"], t["part"], t["sort"], t["desc"], fn, t["N"], True)
        assert (order, ranking) == t["out"][fn], FN_NAMES[fn]
        bare = REFS[ref](t["rows"], t["part"], t["sort"], t["desc"], fn, t["N"], False)
        assert bare == (t["out"][fn][0], None)


@pytest.mark.parametrize("name", sorted(TABLES))
def test_vec_reference_by_hand(name):
    t = TABLES[name]
    for fn in FNS:
        order, ranking = ref_topn_ranking_vec(table_cols(t["rows"]), t["part"], t["sort"],
                                              t["desc"], fn, t["N"], True)
        assert (order.tolist(), ranking.tolist()) == t["out"][fn], FN_NAMES[fn]


# --------------------------------------------------------------------------
# the three references agree on random inputs
# --------------------------------------------------------------------------
SHAPES = (([0], [1], [0]), ([0], [1], [1]), ([], [1], [1]), ([0], [], []), ([], [], []),
          ([0, 1], [1, 3], [1, 0]))


def random_rows(n, seed, pkind="i64", skind="f64"):
    from test_gpu_filter_matrix import rows_of
    from test_window_reference import random_cols
    cols = random_cols(n, seed, pkind, skind)
    return cols, rows_of(cols)


@pytest.mark.parametrize("n", [1, 2, 65, 700])
@pytest.mark.parametrize("pkind,skind", [("i64", "f64"), ("f64", "i32"), ("bool", "i8")])
def test_references_agree_on_random_inputs(n, pkind, skind):
    cols, rows = random_rows(n, 300 + n, pkind, skind)
    for part, sort, desc in SHAPES:
        for fn in FNS:
            for N in (1, 2, 5, n + 1):
                exp = ref_topn_ranking(rows, part, sort, desc, fn, N, True)
                assert independent_topn_ranking(rows, part, sort, desc, fn, N, True) == exp
                order, ranking = ref_topn_ranking_vec(cols, part, sort, desc, fn, N, True)
                assert (order.tolist(), ranking.tolist()) == exp


def test_every_partition_keeps_a_row():
    """m = 0 cannot happen with N >= 1: the first row of a partition ranks 1"""
    from test_gpu_ordering_matrix import canon_key
    _, rows = random_rows(500, 9)
    for fn in FNS:
        order, ranking = ref_topn_ranking(rows, [0], [1], [0], fn, 1, True)
        parts = {canon_key((r[0],)) for r in rows}
        assert {canon_key((rows[i][0],)) for i in order} == parts
        assert len(order) >= len(parts) and set(ranking) == {1}


# --------------------------------------------------------------------------
# pruning: the algorithm of DESIGN.md §6i without a GPU
# --------------------------------------------------------------------------
def pruned_topn_ranking(rows, sizes, part, sort, desc, fn, N, emit):
    """cut `retained + next page` after every page, then once more with the
    ranking; the retained rows go FIRST, so ties keep input order"""
    retained, at = [], 0                   # input row indices
    for size in sizes:
        held = retained + list(range(at, at + size))
        at += size
        order, _ = ref_topn_ranking([rows[i] for i in held], part, sort, desc, fn, N, False)
        retained = [held[j] for j in order]
    assert at == len(rows)
    order, ranking = ref_topn_ranking([rows[i] for i in retained], part, sort, desc, fn, N, emit)
    return [retained[j] for j in order], ranking


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("fn", FNS, ids=FN_NAMES)
def test_pruning_page_by_page_equals_the_whole_input(fn, seed):
    r = np.random.default_rng(seed)
    n = 400
    _, rows = random_rows(n, 40 + seed, "i16", "f64")
    cuts = np.sort(r.integers(0, n + 1, 9))
    sizes = np.diff(np.concatenate(([0], cuts, [n]))).tolist()      # zero-row pages among them
    for part, sort, desc in SHAPES:
        for N in (1, 3, 64, n + 1):
            whole = ref_topn_ranking(rows, part, sort, desc, fn, N, True)
            assert pruned_topn_ranking(rows, sizes, part, sort, desc, fn, N, True) == whole
            assert (pruned_topn_ranking(rows, sizes, part, sort, desc, fn, N, False) ==
                    (whole[0], None))


def test_a_cut_row_never_comes_back():
    """a row's ranking over a subset never exceeds its ranking over a
    superset that keeps the subset's rows first among ties"""
    _, rows = random_rows(300, 77)
    for fn in FNS:
        sub = list(range(0, 300, 2))
        o_sub, r_sub = ref_topn_ranking([rows[i] for i in sub], [0], [1], [0], fn, 10 ** 9, True)
        o_all, r_all = ref_topn_ranking(rows, [0], [1], [0], fn, 10 ** 9, True)
        whole = dict(zip(o_all, r_all))
        for j, rk in zip(o_sub, r_sub):
            assert rk <= whole[sub[j]]


# --------------------------------------------------------------------------
# the rank cut's placement
# --------------------------------------------------------------------------
def rank_cut_model(keep, chunk):
    """k_rcut_count, the scan of the counts, k_rcut_place: a 'wave' per chunk
    walks 64-row groups; a kept row lands at the chunk's base + the keeps in
    the lanes below it"""
    n = len(keep)
    nchunks = -(-n // chunk)

    def ballots(c):
        lo, hi = c * chunk, min((c + 1) * chunk, n)
        for g in range(lo, hi, 64):
            b = 0
            for lane in range(64):
                if g + lane < hi and keep[g + lane]:
                    b |= 1 << lane
            yield g, b

    counts = [sum(bin(b).count("1") for _, b in ballots(c)) for c in range(nchunks)]
    scanned = np.cumsum(counts).tolist()               # inclusive, as run_wscan gives it
    out = [None] * (scanned[-1] if scanned else 0)
    for c in range(nchunks):
        base = scanned[c - 1] if c else 0
        for g, b in ballots(c):
            for lane in range(64):
                if b >> lane & 1:
                    at = base + bin(b & ((1 << lane) - 1)).count("1")
                    assert out[at] is None
                    out[at] = g + lane
            base += bin(b).count("1")
    return out


def cut_patterns(n, chunk, seed):
    pos = np.arange(n)
    r = np.random.default_rng(seed)
    return {"all": np.ones(n, bool), "none_but_first": pos == 0,
            "lane0": pos % 64 == 0, "lane63": pos % 64 == 63,
            "empty_chunk": (pos // chunk) % 2 == 0,     # nothing kept in every other chunk
            "last_only": pos == n - 1, "random": r.random(n) < 0.3}


def test_rank_cut_placement_model():
    c = source_constants()["WSCAN_CHUNK"]
    sizes = (1, 2, 63, 64, 65, c - 1, c, c + 1, 2 * c + 1, 64 * c + 1)
    for n in sizes:
        names = ("all", "lane63", "empty_chunk", "random") if n > 4 * c else None
        for name, keep in cut_patterns(n, c, n).items():
            if names and name not in names:
                continue
            assert rank_cut_model(keep.tolist(), c) == np.flatnonzero(keep).tolist(), (n, name)


# --------------------------------------------------------------------------
# constants
# --------------------------------------------------------------------------
def test_constants_match_the_header():
    """trino_amd.ops RANKING_* against include/trino_gpu.h, and both against
    the Window's function ids, which the references here pass to ref_window"""
    header = open(os.path.join(_ROOT, "include", "trino_gpu.h")).read()
    from trino_amd import ops
    for name, val in (("ROW_NUMBER", ROW_NUMBER), ("RANK", RANK), ("DENSE_RANK", DENSE_RANK)):
        m = re.search(rf"TG_RANKING_{name} = (\d+)", header)
        assert m and int(m.group(1)) == val == getattr(ops, f"RANKING_{name}"), name
        assert getattr(ops, f"WIN_{name}") == val
    assert "tg_topn_ranking_create" in header


def test_gpu_matrix_sizes_follow_the_chunk():
    import test_gpu_topn_ranking_matrix as m
    c = source_constants()["WSCAN_CHUNK"]
    assert m.C == c and c % 64 == 0
    assert m.EDGE_SIZES == (1, 2, 63, 64, 65, c - 1, c, c + 1, 2 * c + 1)
    assert m.WAVE_CARRIES_ROWS == 64 * c + 1
