"""Reference of OrderBy / TopN-with-VARCHAR (tg_order_by_create,
tg_topn_create_ex; include/trino_gpu.h) and of the VARCHAR sort image of
order_pages (trino_amd/csrc/sort.hip). No GPU.

ref_order_by is the exact reference the GPU matrix (test_gpu_order_by_matrix)
compares against: stable passes from the least significant key. Here it is
checked against a second, independent comparator sort.

refine_ranks is a plain-Python model of the chunk refinement the device runs:
dense ranks of byte strings from 8-byte big-endian chunks, one more round on
the lengths. It is checked against sorted(set(...)), with its round bound.

tg_varchar_chunk_host runs the very cell function the kernel runs
(csrc/var_keys.h) and is checked against int.from_bytes.
"""
import ctypes
import functools
import itertools
import math
import os
import random

from test_gpu_ordering_matrix import canon_key

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "trino_amd", "libtrino_gpu.so")
TG_ERR_INVALID_ARG = 1


def _built():
    if not os.path.exists(SO):
        import __graft_entry__
        __graft_entry__.build()


# --------------------------------------------------------------------------
# the operator's reference
# --------------------------------------------------------------------------
def _value_key(v):
    """a comparable stand-in for a non-NULL cell: bytes compare as bytes
    (unsigned, a proper prefix first), numbers numerically with one NaN above
    everything and one zero"""
    c = canon_key((v,))[0]
    return (1, 0) if c == "nan" else (0, c)


def ref_order_by(rows, sort, desc, limit=None):
    """Input row indices in output order. rows: tuples of cells (None = NULL,
    bytes for VARCHAR); sort: key channels, most significant first; desc: 0 =
    ASC nulls last, 1 = DESC nulls first. Stable passes from the least
    significant key: whole-key ties keep input order. ASC sorts by (is_null,
    value); DESC sorts the same pair with reverse=True, which puts NULL first
    and keeps ties in input order."""
    order = list(range(len(rows)))
    for ch, d in reversed(list(zip(sort, desc))):
        def key(i, ch=ch):
            v = rows[i][ch]
            return (1,) if v is None else (0, _value_key(v))
        order.sort(key=key, reverse=bool(d))
    return order if limit is None else order[:limit]


def _cmp_cells(a, b, d):
    """three-way compare of two cells of one key channel, written without
    ref_order_by's helpers"""
    if a is None or b is None:
        if a is None and b is None:
            return 0
        first_is_a = (a is None) == bool(d)      # DESC: NULL first; ASC: NULL last
        return -1 if first_is_a else 1
    if isinstance(a, bytes):
        n = min(len(a), len(b))
        c = 0
        for x, y in zip(a[:n], b[:n]):
            if x != y:
                c = -1 if x < y else 1
                break
        if c == 0:
            c = (len(a) > len(b)) - (len(a) < len(b))
    elif isinstance(a, float):
        an, bn = a != a, b != b
        c = (an - bn) if (an or bn) else (a > b) - (a < b)      # -0.0 == 0.0 in Python too
    else:
        c = (a > b) - (a < b)
    return -c if d else c


def cmp_order_by(rows, sort, desc, limit=None):
    def cmp(i, j):
        for ch, d in zip(sort, desc):
            c = _cmp_cells(rows[i][ch], rows[j][ch], d)
            if c:
                return c
        return (i > j) - (i < j)
    order = sorted(range(len(rows)), key=functools.cmp_to_key(cmp))
    return order if limit is None else order[:limit]


ADVERSARIAL = [b"", b"\0", b"\0\0", b"a", b"a\0", b"ab", b"\x7f", b"\x80", b"\xff"]


def test_documented_string_order():
    rows = [(s,) for s in reversed(ADVERSARIAL)]
    got = [rows[i][0] for i in ref_order_by(rows, [0], [0])]
    assert got == ADVERSARIAL
    got = [rows[i][0] for i in ref_order_by(rows, [0], [1])]
    assert got == ADVERSARIAL[::-1]


def test_null_placement_and_ties_keep_input_order():
    rows = [(b"", 0), (None, 1), (b"a", 2), (None, 3), (b"", 4), (b"a", 5)]
    assert ref_order_by(rows, [0], [0]) == [0, 4, 2, 5, 1, 3]      # ASC nulls last
    assert ref_order_by(rows, [0], [1]) == [1, 3, 2, 5, 0, 4]      # DESC nulls first
    assert ref_order_by(rows, [0], [1], limit=3) == [1, 3, 2]
    nums = [(0.0,), (-0.0,), (math.nan,), (None,), (-math.nan,), (math.inf,)]
    assert ref_order_by(nums, [0], [0]) == [0, 1, 5, 2, 4, 3]
    assert ref_order_by(nums, [0], [1]) == [3, 2, 4, 5, 0, 1]


def test_ref_order_by_against_comparator_sort():
    r = random.Random(7)
    strs = ADVERSARIAL + [b"a" * 8, b"a" * 8 + b"\0", b"a" * 9, None]
    ints = [-2, -1, 0, 1, 2 ** 40, None]
    dbls = [0.0, -0.0, 1.5, -1.5, math.nan, math.inf, -math.inf, None]
    for case in range(300):
        n = r.randrange(0, 40)
        rows = [(r.choice(strs), r.choice(ints), r.choice(dbls), r.choice(strs))
                for _ in range(n)]
        k = r.randrange(1, 5)
        sort = [r.randrange(4) for _ in range(k)]
        desc = [r.randrange(2) for _ in range(k)]
        limit = r.choice([None, 1, max(n - 1, 1), n + 1])
        assert ref_order_by(rows, sort, desc, limit) == cmp_order_by(rows, sort, desc, limit), \
            (case, sort, desc, limit)


# --------------------------------------------------------------------------
# the rank-refinement model of the VARCHAR image
# --------------------------------------------------------------------------
def chunk(s, r):
    return int.from_bytes(s[8 * r:8 * r + 8].ljust(8, b"\0"), "big")


def refine_ranks(strings):
    """(dense ranks, rounds run). Each round: stable sort of perm by the
    round's image, stable sort by the current rank, a flag where (rank, image)
    changes, a running sum of the flags as the new ranks; `more` where two
    adjacent positions tie and either string goes on past the bytes seen."""
    n = len(strings)
    rank = [0] * n
    perm = list(range(n))

    def one_round(image, seen_bytes):
        perm.sort(key=lambda i: image[i])
        perm.sort(key=lambda i: rank[i])
        flags, more = [0] * n, False
        for p in range(1, n):
            a, b = perm[p - 1], perm[p]
            flags[p] = int(rank[a] != rank[b] or image[a] != image[b])
            if not flags[p] and (len(strings[a]) > seen_bytes or len(strings[b]) > seen_bytes):
                more = True
        new = list(itertools.accumulate(flags))
        for p in range(n):
            rank[perm[p]] = new[p]
        return more

    rounds = 0
    while True:
        more = one_round([chunk(s, rounds) for s in strings], 8 * (rounds + 1))
        rounds += 1
        if not more:
            break
    one_round([len(s) for s in strings], math.inf)
    return rank, rounds + 1


def check_ranks(strings):
    rank, rounds = refine_ranks(strings)
    dense = {s: k for k, s in enumerate(sorted(set(strings)))}
    assert rank == [dense[s] for s in strings], strings
    max_len = max((len(s) for s in strings), default=0)
    assert rounds <= max(1, -(-max_len // 8)) + 1, (rounds, max_len, strings)


def test_refinement_exhaustive_three_byte_alphabet():
    alphabet = (b"\0", b"a", b"b")
    every = [b"".join(t) for k in range(4) for t in itertools.product(alphabet, repeat=k)]
    assert len(every) == 40
    check_ranks(every)
    check_ranks(every[::-1])
    r = random.Random(3)
    for _ in range(200):
        check_ranks([r.choice(every) for _ in range(r.randrange(1, 60))])
    for pair in itertools.product(every, repeat=2):
        check_ranks(list(pair))


def test_refinement_shared_prefix_family():
    r = random.Random(11)
    tail_bytes = (0x00, ord("a"), ord("b"), 0x80, 0xff)
    for case in range(3000):
        plen = r.choice((0, 7, 8, 9, 16, 23))
        prefix = bytes(r.choice(tail_bytes) for _ in range(plen))
        strings = [prefix[:r.choice((plen, plen, plen, r.randrange(plen + 1)))] +
                   bytes(r.choice(tail_bytes) for _ in range(r.randrange(0, 11)))
                   for _ in range(r.randrange(1, 14))]
        check_ranks(strings)


def test_refinement_round_count_is_set_by_where_strings_separate():
    """long strings that differ in their first chunk need one chunk round"""
    strings = [bytes([65 + k]) + b"x" * 200 for k in range(20)]
    assert refine_ranks(strings)[1] == 2
    strings = [b"p" * 64 + bytes([65 + k]) for k in range(20)]
    assert refine_ranks(strings)[1] == 9 + 1


# --------------------------------------------------------------------------
# the cell function the kernel runs
# --------------------------------------------------------------------------
def _chunk_fn():
    _built()
    lib = ctypes.CDLL(SO)
    fn = lib.tg_varchar_chunk_host
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32,
                   ctypes.POINTER(ctypes.c_uint64)]
    return fn


def test_varchar_chunk_host_against_int_from_bytes():
    fn = _chunk_fn()
    out = ctypes.c_uint64(1)
    patterns = (bytes((0x80 + 7 * i) & 0xff for i in range(17)),      # bytes >= 0x80
                bytes(17),                                            # all 0x00
                bytes((0, 0xff, 0x7f, 0x80, 0, 1) * 3)[:17],
                b"abcdefghijklmnopq")
    for pat in patterns:
        for n in range(18):
            s = pat[:n]
            for rnd in range(3):
                padded = s[8 * rnd:8 * rnd + 8].ljust(8, b"\0")
                out.value = 1
                assert fn(s if n else None, n, rnd, ctypes.byref(out)) == 0
                assert out.value == int.from_bytes(padded, "big") == chunk(s, rnd), (s, rnd)
    # chunk order is byte order of the window
    assert fn(b"\x80", 1, 0, ctypes.byref(out)) == 0
    hi = out.value
    assert fn(b"\x7f\xff", 2, 0, ctypes.byref(out)) == 0
    assert out.value < hi


def test_varchar_chunk_host_rejections():
    fn = _chunk_fn()
    out = ctypes.c_uint64(5)
    ref = ctypes.byref(out)
    assert fn(None, 0, 0, ref) == 0 and out.value == 0
    assert fn(None, 0, 2, ref) == 0 and out.value == 0
    out.value = 5
    for args in ((b"a", 1, 0, None), (b"a", -1, 0, ref), (b"a", 1, -1, ref),
                 (None, 1, 0, ref)):
        assert fn(*args) == TG_ERR_INVALID_ARG
    assert out.value == 5


def test_ops_wrappers_exist():
    """the public interface: ops.order_by, ops.topn_ex and the chunk hook"""
    _built()
    from trino_amd import ops
    assert callable(ops.order_by) and callable(ops.topn_ex)
    assert ops.varchar_chunk_host(b"ab", 0) == int.from_bytes(b"ab" + bytes(6), "big")
    assert ops.varchar_chunk_host(b"", 1) == 0
