"""Reference for the lookup join's residual filter (`ON a.k = b.k AND
<filter>`), and its host side checks (no GPU).

ref_join_filtered(build_rows, probe_rows, bkeys, pkeys, prog, outer) returns
(pairs, unmatched_build_rows):
 - the candidates are the pairs of test_gpu_join_matrix.ref_join over the key
   cells, in its order (probe rows ascending, the build rows of one probe row
   descending);
 - a candidate is a match iff test_gpu_filter_matrix.ref_keep(prog,
   probe_cells + build_cells) holds, i.e. the filter is non-NULL and non-zero;
   column index c names probe channel c when c < len(probe row), else build
   channel c - len(probe row);
 - `pairs` are the matches in candidate order; with `outer`, a probe row left
   without a match (NULL key, no equal key, or every candidate failed) gives
   one (i, None) at its place;
 - `unmatched_build_rows` are, ascending, the build rows in no match: what
   the lookup-outer operator must emit after a RIGHT / FULL join.

ref_join_filtered_vec is the vectorised twin for single BIGINT keys on top of
ref_join_vec; the filter comes as a numpy predicate over the candidate index
arrays. Both are checked here by hand-written cases, against a nested-loop
join that shares no code with ref_join, and against each other.
tests/test_gpu_join_filter_matrix.py imports them.
"""
import ctypes
import os

import numpy as np

from test_gpu_filter_matrix import ref_keep
from test_gpu_join_matrix import ref_join, ref_join_vec
from test_outer_join_reference import _sql_equal

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_ROOT, "trino_amd", "libtrino_gpu.so")


def _key(row, channels):
    return tuple(row[c] for c in channels)


def ref_join_filtered(build_rows, probe_rows, bkeys, pkeys, prog, outer):
    bk = [_key(r, bkeys) for r in build_rows]
    pk = [_key(r, pkeys) for r in probe_rows]
    kept = [(i, r) for i, r in ref_join(bk, pk, False)
            if ref_keep(prog, tuple(probe_rows[i]) + tuple(build_rows[r]))]
    pairs, at = [], 0
    for i in range(len(probe_rows)):
        start = at
        while at < len(kept) and kept[at][0] == i:
            at += 1
        pairs.extend(kept[start:at])
        if outer and at == start:
            pairs.append((i, None))
    assert at == len(kept)
    matched = {r for _, r in kept}
    return pairs, [r for r in range(len(build_rows)) if r not in matched]


def ref_join_filtered_vec(bk, bvalid, pk, pvalid, pred, outer):
    """single BIGINT keys; pred(op, ob) -> bool array over the candidate index
    arrays (True = the filter is non-NULL and non-zero). Returns (probe rows,
    build rows with -1 for the NULL side, unmatched build rows), int64."""
    op, ob = ref_join_vec(bk, bvalid, pk, pvalid)
    keep = np.asarray(pred(op, ob), bool)
    assert keep.shape == op.shape
    op, ob = op[keep], ob[keep]
    unmatched = np.flatnonzero(np.bincount(ob, minlength=len(bk)) == 0).astype(np.int64)
    if outer:
        lone = np.flatnonzero(np.bincount(op, minlength=len(pk)) == 0).astype(np.int64)
        aop = np.concatenate([op, lone])
        aob = np.concatenate([ob, np.full(len(lone), -1, np.int64)])
        order = np.argsort(aop, kind="stable")    # a lone row has no other entry
        op, ob = aop[order], aob[order]
    return op, ob, unmatched


# --------------------------------------------------------------------------
# an independent nested-loop join
# --------------------------------------------------------------------------
def nested_loop_filtered(build_rows, probe_rows, bkeys, pkeys, prog, outer):
    pairs, matched = [], set()
    for i, p in enumerate(probe_rows):
        hit = False
        for r in range(len(build_rows) - 1, -1, -1):
            b = build_rows[r]
            if _sql_equal(_key(p, pkeys), _key(b, bkeys)) and \
                    ref_keep(prog, tuple(p) + tuple(b)):
                pairs.append((i, r))
                matched.add(r)
                hit = True
        if outer and not hit:
            pairs.append((i, None))
    return pairs, [r for r in range(len(build_rows)) if r not in matched]


C = lambda i: ("col", i)           # noqa: E731
I = lambda v: ("i64", v)           # noqa: E731


def test_by_hand_q21_form():
    """probe (key, x), build (key, y): ON key = key AND x <> y"""
    build = [(7, 1), (7, 2), (3, 5), (7, None), (None, 9), (4, 4)]
    probe = [(7, 1), (3, 5), (7, None), (None, 1), (8, 0), (4, 5)]
    ne = (C(1), C(2 + 1), "ne")
    pairs, un = ref_join_filtered(build, probe, [0], [0], ne, False)
    # probe 0: candidates 3, 1, 0 -> NULL, 1 <> 2 kept, 1 <> 1 fails
    assert pairs == [(0, 1), (5, 5)]
    assert un == [0, 2, 3, 4]
    pairs, un = ref_join_filtered(build, probe, [0], [0], ne, True)
    assert pairs == [(0, 1), (1, None), (2, None), (3, None), (4, None), (5, 5)]
    assert un == [0, 2, 3, 4]


def test_by_hand_constants_and_order():
    build = [(1, 10), (1, 20), (1, 30), (2, 40)]
    probe = [(1, 0), (2, 0), (5, 0)]
    pairs, un = ref_join_filtered(build, probe, [0], [0], (I(1),), True)
    assert pairs == [(0, 2), (0, 1), (0, 0), (1, 3), (2, None)] and un == []
    assert pairs == ref_join([(r[0],) for r in build], [(r[0],) for r in probe], True)
    pairs, un = ref_join_filtered(build, probe, [0], [0], (I(0),), True)
    assert pairs == [(0, None), (1, None), (2, None)] and un == [0, 1, 2, 3]
    pairs, un = ref_join_filtered(build, probe, [0], [0], (I(0),), False)
    assert pairs == [] and un == [0, 1, 2, 3]
    # build.v BETWEEN 15 AND 30: middle and first candidate only, order kept
    btw = (C(2 + 1), I(15), I(30), "between")
    pairs, un = ref_join_filtered(build, probe, [0], [0], btw, False)
    assert pairs == [(0, 2), (0, 1)] and un == [0, 3]
    assert ref_join_filtered([], probe, [0], [0], btw, True) == \
        ([(0, None), (1, None), (2, None)], [])
    assert ref_join_filtered(build, [], [0], [0], btw, True) == ([], [0, 1, 2, 3])


_PROGS = [
    (C(1), C(3 + 1), "ne"),
    (C(3 + 2), C(1), C(2), "between"),
    (C(1), C(3 + 1), "div", I(0), "ge"),
    (C(1), C(3 + 1), "eq", "not"),
    (C(1), C(3 + 1), "eq", C(2), I(1), "lt", "or"),
    (I(1),), (I(0),),
]


def _random_rows(r, n, dsize):
    dom = [None, -2, -1, 0, 1, 2, 3][:max(dsize, 2)]
    pick = lambda: dom[int(r.integers(0, len(dom)))]     # noqa: E731
    return [(pick(), pick(), pick()) for _ in range(n)]


def test_equals_nested_loop():
    r = np.random.default_rng(41)
    partial = lone = 0
    for case in range(420):
        nb = int(r.integers(0, 20)) if case % 9 else 0
        m = int(r.integers(0, 20)) if case % 11 else 0
        dsize = int(r.integers(2, 8))
        build, probe = _random_rows(r, nb, dsize), _random_rows(r, m, dsize)
        prog = _PROGS[case % len(_PROGS)]
        for outer in (False, True):
            got = ref_join_filtered(build, probe, [0], [0], prog, outer)
            assert got == nested_loop_filtered(build, probe, [0], [0], prog, outer), \
                (build, probe, prog, outer)
        cands = ref_join([(b[0],) for b in build], [(p[0],) for p in probe], False)
        kept = [p for p in got[0] if p[1] is not None]
        partial += 0 < len(kept) < len(cands)
        lone += len({i for i, _ in cands} - {i for i, _ in kept}) > 0
    assert partial > 100 and lone > 100


def test_vectorised_twin_equals_ref():
    """single BIGINT key, filter probe.x <> build.y with NULLs on both sides"""
    r = np.random.default_rng(42)
    for case in range(300):
        nb = int(r.integers(0, 40)) if case % 9 else 0
        m = int(r.integers(0, 40)) if case % 11 else 0
        dsize = int(r.integers(1, 12))
        bk = r.integers(-dsize, dsize, nb).astype(np.int64)
        pk = r.integers(-dsize, dsize, m).astype(np.int64)
        bv = None if case % 3 == 0 else r.random(nb) > 0.2
        pv = None if case % 4 == 0 else r.random(m) > 0.2
        y, yv = r.integers(0, 3, nb), r.random(nb) > 0.2
        x, xv = r.integers(0, 3, m), r.random(m) > 0.2
        build = [(int(bk[i]) if bv is None or bv[i] else None,
                  int(y[i]) if yv[i] else None) for i in range(nb)]
        probe = [(int(pk[i]) if pv is None or pv[i] else None,
                  int(x[i]) if xv[i] else None) for i in range(m)]
        pred = lambda op, ob: xv[op] & yv[ob] & (x[op] != y[ob])   # noqa: E731
        for outer in (False, True):
            pairs, un = ref_join_filtered(build, probe, [0], [0],
                                          (C(1), C(2 + 1), "ne"), outer)
            op, ob, vun = ref_join_filtered_vec(bk, bv, pk, pv, pred, outer)
            assert op.tolist() == [p for p, _ in pairs]
            assert ob.tolist() == [-1 if b is None else b for _, b in pairs]
            assert vun.tolist() == un


def test_join_filter_in_library_and_wrapper():
    """the C entry point resolves in the built library and ops.lookup_join
    takes filter= (neither does before the join filter was added)"""
    import inspect
    if not os.path.exists(_SO):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_SO)
    assert hasattr(lib, "tg_lookup_join_create_filtered")
    from trino_amd import ops
    assert "filter" in inspect.signature(ops.lookup_join).parameters
    assert inspect.signature(ops.lookup_join).parameters["filter"].default is None
    assert "build channel" in ops.lookup_join.__doc__
