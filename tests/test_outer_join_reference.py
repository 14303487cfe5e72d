"""Reference for the build-outer half of RIGHT and FULL joins, and its host
side checks (no GPU).

ref_unmatched(build_keys, probe_keys) returns, ascending, the build rows that
appear in no pair of test_gpu_join_matrix.ref_join(build_keys, probe_keys,
False): the rows the lookup-outer operator must emit. A build row whose key
has a NULL or a NaN component is always among them. ref_unmatched_vec is the
vectorised twin for single BIGINT keys on top of ref_join_vec.

Both are checked here against a plain nested-loop join that shares no code
with ref_join. tests/test_gpu_outer_join_matrix.py imports them.
"""
import ctypes
import os

import numpy as np

from test_gpu_join_matrix import ref_join, ref_join_vec

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_ROOT, "trino_amd", "libtrino_gpu.so")


def ref_unmatched(build_keys, probe_keys):
    matched = {b for _, b in ref_join(build_keys, probe_keys, False)}
    return [r for r in range(len(build_keys)) if r not in matched]


def ref_unmatched_vec(bk, bvalid, pk, pvalid):
    """ref_unmatched for single BIGINT keys: ascending int64 build rows"""
    _, ob = ref_join_vec(bk, bvalid, pk, pvalid)
    hits = np.bincount(ob, minlength=len(bk))
    rows = np.flatnonzero(hits == 0).astype(np.int64)
    assert np.array_equal(rows, np.setdiff1d(np.arange(len(bk), dtype=np.int64), ob))
    return rows


# --------------------------------------------------------------------------
# an independent nested-loop join
# --------------------------------------------------------------------------
def _sql_equal(a, b):
    """SQL `=` on key tuples: a NULL component is never equal; floats by IEEE
    == (so -0.0 == 0.0 and NaN != NaN); everything else by value"""
    for x, y in zip(a, b):
        if x is None or y is None:
            return False
        if not x == y:
            return False
    return True


def nested_loop_unmatched(build_keys, probe_keys):
    return [r for r, bkey in enumerate(build_keys)
            if not any(_sql_equal(bkey, pkey) for pkey in probe_keys)]


NAN = float("nan")
_DOMAINS = {
    "int": [None, -3, 0, 1, 2, 7, 2 ** 40],
    "float": [None, NAN, -0.0, 0.0, 1.5, -1.5, float("inf")],
    "bytes": [None, b"", b"a", b"ab", b"a\0"],
}


def _random_keys(r, n, kinds, domain_size):
    cols = []
    for kind in kinds:
        dom = _DOMAINS[kind]
        dom = [dom[i] for i in r.permutation(len(dom))[:domain_size]]
        cols.append([dom[i] for i in r.integers(0, len(dom), n)])
    return list(zip(*cols)) if n else []


def test_ref_unmatched_by_hand():
    build = [(7,), (3,), (7,), (None,), (5,)]
    assert ref_unmatched(build, [(7,), (4,), (None,)]) == [1, 3, 4]
    assert ref_unmatched(build, []) == [0, 1, 2, 3, 4]
    assert ref_unmatched([], [(1,)]) == []
    assert ref_unmatched(build, [(7,), (3,), (5,)]) == [3]
    # NaN never matches, itself included; -0.0 matches 0.0
    assert ref_unmatched([(NAN,), (0.0,), (-0.0,), (1.5,)], [(NAN,), (-0.0,)]) == [0, 3]
    # a NULL component anywhere in the key
    assert ref_unmatched([(1, None), (1, 2), (None, 2)], [(1, 2), (1, None)]) == [0, 2]


def test_ref_unmatched_equals_nested_loop():
    r = np.random.default_rng(31)
    shapes = [("int",), ("float",), ("bytes",), ("int", "float"), ("bytes", "int")]
    seen_nonempty = seen_empty_side = 0
    for case in range(400):
        kinds = shapes[case % len(shapes)]
        nb = int(r.integers(0, 25)) if case % 9 else 0
        m = int(r.integers(0, 25)) if case % 11 else 0
        dsize = int(r.integers(1, 8))
        build = _random_keys(r, nb, kinds, dsize)
        probe = _random_keys(r, m, kinds, dsize)
        got = ref_unmatched(build, probe)
        assert got == nested_loop_unmatched(build, probe), (build, probe)
        assert got == sorted(got)
        seen_nonempty += bool(got) and len(got) < nb
        seen_empty_side += (nb == 0) or (m == 0)
    assert seen_nonempty > 100 and seen_empty_side > 40


def test_vectorised_twin_equals_ref_unmatched():
    r = np.random.default_rng(32)
    for case in range(300):
        nb = int(r.integers(0, 40)) if case % 9 else 0
        m = int(r.integers(0, 40)) if case % 11 else 0
        dsize = int(r.integers(1, 30))
        bk = r.integers(-dsize, dsize, nb).astype(np.int64)
        pk = r.integers(-dsize, dsize, m).astype(np.int64)
        bv = None if case % 3 == 0 else r.random(nb) > 0.2
        pv = None if case % 4 == 0 else r.random(m) > 0.2
        bkeys = [(int(k) if bv is None or bv[i] else None,) for i, k in enumerate(bk)]
        pkeys = [(int(k) if pv is None or pv[i] else None,) for i, k in enumerate(pk)]
        ref = ref_unmatched(bkeys, pkeys)
        assert ref_unmatched_vec(bk, bv, pk, pv).tolist() == ref
        assert ref == nested_loop_unmatched(bkeys, pkeys)


def test_lookup_outer_in_library_and_wrapper():
    """the C entry point resolves in the built library and the Python wrapper
    exists (neither does before the lookup-outer operator was added)"""
    if not os.path.exists(_SO):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_SO)
    assert hasattr(lib, "tg_lookup_outer_create")
    from trino_amd import ops
    assert callable(ops.lookup_outer)
    assert "2" in ops.lookup_join.__doc__ and "FULL" in ops.lookup_join.__doc__
