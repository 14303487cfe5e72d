"""Text-match and distinct parity matrix: tg_varchar_like_flags and
tg_pool_like_flags (trino_amd/csrc/tpchgen.hip + like_match.h),
tg_mark_distinct_create and the adaptive partial-aggregation pass-through
(ops_groupby.hip) and tg_dedup_i64 (sort.hip) against exact references
written here in plain Python over bytes, int and None.

References:
  - ref_like(pattern, text): a segment matcher on bytes. '%' is the only
    wildcard; a pattern without '%' is equality; '' matches only b''.
  - ref_mark_distinct(rows): a set of canonical key tuples. NULL is a key
    value, every NaN is one key, -0.0 is 0.0, VARCHAR compares by bytes and
    b'' is not NULL.
  - ref_partial_state(fn, cell, scale_pow): the per-row partial state of the
    pass-through (the combine-neutral element for a NULL cell).
  - FINAL over partial pages is compared with the SINGLE reference of
    tests/test_gpu_aggregation_matrix.py (imported, not rewritten).

Comparison: byte for byte / bit for bit everywhere; no tolerance.

Every LIKE case expects both verdicts among its flags, so that a kernel
that writes a constant cannot pass. Two kinds of pattern cannot: '%' and
'%%' (every text matches) and a segment that occurs nowhere in the pool
(no slice matches); LIKE_ALL_ONE and the pool's NOWHERE pattern name them.

Host-side checks of these references and shapes are in
tests/test_oracle_units.py::TestTextDistinctMatrixHost (no GPU); the matcher
itself is checked exhaustively without a GPU in tests/test_abi_cpu.py.
"""
import ctypes
import functools
import itertools
import math
import os
import random
import re
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "trino_amd", "csrc")

TG_OK, TG_ERR_INVALID_ARG, TG_ERR_UNSUPPORTED = 0, 1, 6


# --------------------------------------------------------------------------
# constants of the code under test, parsed from its sources
# --------------------------------------------------------------------------
@functools.lru_cache(None)
def source_constants():
    like = open(os.path.join(_CSRC, "like_match.h")).read()
    gen = open(os.path.join(_CSRC, "tpchgen.hip")).read()
    common = open(os.path.join(_CSRC, "common.h")).read()
    grp = open(os.path.join(_CSRC, "ops_groupby.hip")).read()

    def one(pat, text, conv=int):
        m = re.search(pat, text)
        assert m, pat
        return conv(m.group(1))

    return dict(
        LIKE_MAX_SEGS=one(r"#define LIKE_MAX_SEGS (\d+)", like),
        LIKE_MAX_PAT=one(r"#define LIKE_MAX_PAT (\d+)", like),
        TG_BLOCK=one(r"constexpr int TG_BLOCK = (\d+);", common),
        TG_MAX_BLOCKS=one(r"constexpr int TG_MAX_BLOCKS = (\d+);", common),
        SORTED_SWITCH_SHIFT=one(r"\(n >= \(1 << (\d+)\)\) \? '2' : '0'", gen),
        SORTED_KEY_BITS=one(r"run_sort_pairs_bits\(s, d_so, d_lr, n, (\d+)\)", gen),
        INIT_CAP_SHIFT=one(r"init_table\(1 << (\d+), 1 << \d+\)", grp),
        INIT_GROUPS_SHIFT=one(r"init_table\(1 << \d+, 1 << (\d+)\)", grp),
        LOAD_FACTOR=one(r"ng \+ incoming <= \(int64_t\)\(t\.capacity \* ([0-9.]+)\)",
                        grp, float),
    )


# the values the shapes below assume; TestTextDistinctMatrixHost pins them to
# the parsed ones
LIKE_MAX_SEGS = 4
LIKE_MAX_PAT = 64
GRID_THREADS = 256 * 2048
GRID_N = GRID_THREADS + 257            # 524,545: second grid stride + a tail
SORTED_SWITCH = 1 << 20
INIT_GROUPS = 1 << 16
INIT_CAP = 1 << 17
LOAD_FACTOR = 0.7


# --------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------
def ref_like(pattern, text):
    """pattern, text: bytes. 1 iff text LIKE pattern, '%' the only wildcard."""
    segs = pattern.split(b"%")
    if len(segs) == 1:
        return 1 if text == pattern else 0
    first, last = segs[0], segs[-1]
    if len(text) < len(first) + len(last):
        return 0
    if not text.startswith(first) or not text.endswith(last):
        return 0
    pos, end = len(first), len(text) - len(last)
    for s in segs[1:-1]:
        if not s:
            continue
        j = text.find(s, pos, end)
        if j < 0:
            return 0
        pos = j + len(s)
    return 1


def like_exhaustive_set():
    """every pattern over {a,b,%} of length 0..5 (364); every text over {a,b}
    of length 0..6 plus 300 random ones of 7..40 bytes (427)"""
    pats = [bytes(p) for n in range(6) for p in itertools.product(b"ab%", repeat=n)]
    texts = [bytes(t) for n in range(7) for t in itertools.product(b"ab", repeat=n)]
    r = random.Random(1234)
    texts += [bytes(r.choice(b"ab") for _ in range(r.randint(7, 40)))
              for _ in range(300)]
    return pats, texts


def canon_key_value(v):
    """canonical form of one key cell: None stays None (NULL is a key value),
    every NaN is one key, -0.0 is 0.0, bytes compare as bytes."""
    if isinstance(v, float):
        if v != v:
            return ("nan",)
        if v == 0.0:
            return 0.0
        return v
    return v


def ref_mark_distinct(rows):
    """rows: iterable of key tuples (cells int / float / bytes / None), in
    global row order. Returns the list of 0/1 first-occurrence flags. A float
    cell and an int cell never share a channel, so 1.0 == 1 cannot alias."""
    seen = set()
    out = []
    for r in rows:
        k = tuple(canon_key_value(v) for v in r)
        if k in seen:
            out.append(0)
        else:
            seen.add(k)
            out.append(1)
    return out


I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
(FN_COUNT_STAR, FN_COUNT_COL, FN_SUM_F64, FN_SUM_I64, FN_AVG_F64,
 FN_SUM_F64_EXACT, FN_MIN_I64, FN_MAX_I64) = range(8)


def f64_bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def ref_partial_state(fn, cell, scale_pow=0):
    """The partial-state words of one input cell (None = NULL) as a tuple of
    int64 bit patterns, in channel order: one word, or two for AVG (count,
    sum bits) and SUM_F64_EXACT (lo, hi of the 128-bit int(v * 2**k))."""
    def s64(u):
        u &= (1 << 64) - 1
        return u - (1 << 64) if u >= 1 << 63 else u

    if fn == FN_COUNT_STAR:
        return (1,)
    if fn == FN_COUNT_COL:
        return (0 if cell is None else 1,)
    if fn == FN_SUM_I64:
        return (0 if cell is None else cell,)
    if fn == FN_SUM_F64:
        return (f64_bits(0.0 if cell is None else cell),)
    if fn == FN_MIN_I64:
        return (I64_MAX if cell is None else cell,)
    if fn == FN_MAX_I64:
        return (I64_MIN if cell is None else cell,)
    if fn == FN_AVG_F64:
        return (0, f64_bits(0.0)) if cell is None else (1, f64_bits(cell))
    if fn == FN_SUM_F64_EXACT:
        y = 0 if cell is None else int(cell * 2.0 ** scale_pow)
        assert I64_MIN <= y <= I64_MAX       # the kernel converts through int64
        y &= (1 << 128) - 1
        return (s64(y), s64(y >> 64))
    raise ValueError(fn)


# --------------------------------------------------------------------------
# LIKE cases over a VARCHAR column: (name, [patterns], rows); built once
# --------------------------------------------------------------------------
LIKE_ALL_ONE = (b"%", b"%%")      # match every text: only 1s are expected


def all_strings(alphabet, max_len):
    out = []
    for n in range(max_len + 1):
        out += [bytes(t) for t in itertools.product(alphabet, repeat=n)]
    return out


ANCHOR_PATTERNS = (b"abc", b"abc%", b"%abc", b"%abc%", b"a%c", b"a%b%c",
                   b"%a%b", b"a%b%", b"ab%ab", b"%", b"%%", b"%%a%%",
                   b"%aa%aa%", b"%aab%")
# hand-written verdicts inside the anchor matrix (pattern, text, verdict)
ANCHOR_BY_HAND = ((b"ab%ab", b"ab", 0), (b"ab%ab", b"aba", 0),
                  (b"ab%ab", b"abab", 1), (b"%aa%aa%", b"aaa", 0),
                  (b"%aa%aa%", b"aaaa", 1), (b"%aab%", b"aaab", 1),
                  (b"abc", b"ab", 0), (b"abc", b"", 0), (b"%", b"", 1),
                  (b"abc", b"abcd", 0), (b"abc", b"abc", 1))

SWAR_SEG = b"Qx"
SWAR_PATTERNS = (b"%Qx%", b"%Qx", b"z%Qx%")
SWAR_NEAR = (None, bytes([ord("Q") ^ 0x01]), bytes([ord("Q") ^ 0x80]),
             b"\x00", b"\xff", b"Qy")


def swar_texts():
    """texts of length 1..40 around the segment "Qx": the one true occurrence
    at every position (the last legal start len-2 included), everything
    before it filled with a near-miss of 'Q' (one bit off, the top bit off,
    0x00, 0xFF, or 'Q' followed by a wrong second byte), and for every length
    the same fillers with no occurrence at all and a lone 'Q' as last byte."""
    out = []
    for L in range(1, 41):
        for near in SWAR_NEAR:
            fill = (b"z" if near is None else near) * L
            out.append(fill[:L])                          # no occurrence
            out.append(fill[:L - 1] + b"Q")               # cut off at the end
            for pos in range(0, L - 1):
                out.append(fill[:pos] + SWAR_SEG + b"z" * (L - pos - 2))
    return out


def rows_at_every_alignment(texts):
    """each text at each start alignment 0..7 of the byte array: filler rows
    of length 1 are put in front of it until its offset has that residue"""
    rows, at = [], 0
    for t in texts:
        for a in range(8):
            while at % 8 != a:
                rows.append(b"z")
                at += 1
            rows.append(t)
            at += len(t)
    return rows


BYTES_PATTERNS = (b"%\xc3\xa9%", b"\xc3\xa9%", b"%\xc3\xa9", b"\xc3\xa9",
                  b"a%\xa9", b"%\xff%\x80%", b"\xc3%\xa9")


def grid_rows():
    r = np.random.default_rng(20240)
    lens = r.integers(0, 13, GRID_N)
    lens[0] = lens[GRID_N - 1] = lens[GRID_THREADS] = 0
    data = r.integers(0, 2, int(lens.sum())).astype(np.uint8) + ord("a")
    blob = data.tobytes()
    offs = np.concatenate([[0], np.cumsum(lens)]).tolist()
    return [blob[offs[i]:offs[i + 1]] for i in range(GRID_N)]


@functools.lru_cache(None)
def varchar_like_cases():
    abc5 = all_strings(b"abc", 5)
    ab63 = [b"a" * 62, b"a" * 63, b"a" * 64, b"a" * 62 + b"b", b""]
    four = all_strings(b"abcd", 5)
    return (
        ("no_percent", (b"abc", b"a", b"ab", b"cab"),
         all_strings(b"abc", 4) + [b"abcd", b"abca", b"xabc"]),
        ("empty_pattern", (b"",), [b"", b"a", b"", b"%", b"ab", b"\x00", b""]),
        ("anchor_matrix", ANCHOR_PATTERNS,
         abc5 + [b"ab", b"aba", b"abab", b"aaa", b"aaaa", b"aaab", b"", b"abcd"]),
        ("swar_lanes", SWAR_PATTERNS, rows_at_every_alignment(swar_texts())),
        ("bytes_not_chars", BYTES_PATTERNS,
         all_strings(b"\x00\xc3\xa9a", 4) +
         [b"\xff\x80", b"\xff\x00\x80", b"\x80\xff", b"a\x00\xc3\xa9\x00"]),
        ("limits_accepted", (b"a%b%c%d", b"%a%b%c%d%", b"a" * 63, b"a" * 62 + b"%"),
         four + ab63),
        ("grid_stride", (b"ab%", b"%ab%ba%"), grid_rows()),
    )


def like_case(name):
    for c in varchar_like_cases():
        if c[0] == name:
            return c
    raise KeyError(name)


LIKE_REJECTED = (b"a%b%c%d%e", b"%a%b%c%d%e%", b"a" * 64, b"a" * 63 + b"%",
                 b"_", b"a_b", b"%a_", b"a%b%c%d%_")


# --------------------------------------------------------------------------
# LIKE cases over slices of the dbgen text pool (host-built pool)
# --------------------------------------------------------------------------
POOL_WORDS = (b"special", b"requests")
POOL_NOWHERE = b"%zqzqzq%"           # the segment occurs nowhere in the pool
POOL_FLOATING = (b"%special%requests%", b"%furiousl%")
POOL_PATTERNS = POOL_FLOATING + (b"special%", b"%special", b"special", b"",
                                 POOL_NOWHERE)
N_POOL_RANDOM = 20_000


@functools.lru_cache(None)
def pool_bytes():
    import oracle
    return oracle.text_pool_bytes().tobytes()


def occurrences(pool, word, count, start=0):
    out, at = [], start
    while len(out) < count:
        at = pool.find(word, at)
        assert at >= 0
        out.append(at)
        at += 1
    return out


@functools.lru_cache(None)
def pool_constructed_slices():
    """(offs, lens) int64/int32 arrays: the hand-built slices around real
    occurrences of POOL_WORDS, the pool's two ends, then random slices"""
    pool = pool_bytes()
    P = len(pool)
    sl = []
    for word in POOL_WORDS:
        w = len(word)
        for o in occurrences(pool, word, 40, start=64):
            sl += [(o - 10, 10 + w),        # ends exactly at the occurrence's end
                   (o - 10, 10 + w - 1),    # one byte short of it
                   (o + 1, 40),             # starts one byte after its start
                   (o, 40),                 # starts at it
                   (o, w),                  # is exactly the occurrence
                   (o, w - 1), (o, 0)]
    sl += [(P - 30, 30), (P - 1, 1), (P - 200, 200), (0, 25), (0, 0), (0, 1)]
    last = pool.rfind(POOL_WORDS[0])
    sl += [(last, P - last), (last - 5, P - last + 5)]
    r = np.random.default_rng(77)
    ro = r.integers(0, P - 100, N_POOL_RANDOM)
    rl = r.integers(0, 100, N_POOL_RANDOM)
    offs = np.array([s[0] for s in sl] + ro.tolist(), np.int64)
    lens = np.array([s[1] for s in sl] + rl.tolist(), np.int32)
    return offs, lens


@functools.lru_cache(None)
def pool_switch_slices():
    """2^20 slices; the test runs the first 2^20 - 1 (byte scan) and all of
    them (offset-sorted scan). Groups of rows share one offset and differ in
    length so that the verdict depends on the sort's payload."""
    pool = pool_bytes()
    P = len(pool)
    n = SORTED_SWITCH
    r = np.random.default_rng(78)
    offs = r.integers(0, P - 64, n)
    lens = r.integers(0, 64, n).astype(np.int32)
    occ = occurrences(pool, POOL_WORDS[0], 80, start=1 << 20)
    w = len(POOL_WORDS[0])
    at = 5
    for o in occ:
        for ln in (w + 3, w - 1, 0, w + 20, 2, w + 4):   # same offset o - 3
            offs[at] = o - 3
            lens[at] = ln
            at += 1741                                     # spread over the rows
    offs[n - 1], lens[n - 1] = occ[0] - 3, w + 3          # the row that flips the mode
    offs[0], lens[0] = P - 40, 40
    return offs.astype(np.int64), lens


POOL_SWITCH_PATTERN = b"%special%"


def pool_expected(pattern, offs, lens):
    pool = pool_bytes()
    return np.array([ref_like(pattern, pool[o:o + l])
                     for o, l in zip(offs.tolist(), lens.tolist())], np.uint8)


@functools.lru_cache(None)
def pool_constructed_expected(pattern):
    return pool_expected(pattern, *pool_constructed_slices())


@functools.lru_cache(None)
def pool_switch_expected():
    return pool_expected(POOL_SWITCH_PATTERN, *pool_switch_slices())


def both_verdicts(flags):
    return 0 < int(np.count_nonzero(flags)) < len(flags)


# --------------------------------------------------------------------------
# sorted DISTINCT shapes
# --------------------------------------------------------------------------
DEDUP_BITS = (1, 8, 31, 32, 33, 52, 64)


@functools.lru_cache(None)
def dedup_cases():
    """(name, keys int64 array, bits)"""
    r = np.random.default_rng(5)
    out = [("n0", np.zeros(0, np.int64), 64),
           ("n1", np.array([7], np.int64), 64),
           ("n2_equal", np.array([9, 9], np.int64), 64),
           ("n2_distinct", np.array([9, 3], np.int64), 64),
           ("all_equal", np.full(3001, 12345, np.int64), 64),
           ("sorted_distinct", np.arange(3001, dtype=np.int64) * 3, 64),
           ("reverse_distinct", np.arange(3001, dtype=np.int64)[::-1].copy() * 3, 64)]
    for bits in DEDUP_BITS:
        top = (1 << min(bits, 63)) - 1
        k = np.where(r.integers(0, 2, 1001) == 1, top, 0).astype(np.int64)
        k[0], k[-1] = top, 0
        out.append((f"ends_{bits}", k, bits))
    out.append(("grid", r.integers(0, 200_000, GRID_N).astype(np.int64), 18))
    out.append(("big", r.integers(0, 1 << 40, (1 << 20) + 3).astype(np.int64), 40))
    return tuple(out)


# --------------------------------------------------------------------------
# device plumbing
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


def lib():
    from trino_amd import _lib
    return _lib


def dbuf(sess, nbytes):
    from trino_amd import tpch_queries as tq
    return tq._device_buffer(sess, max(int(nbytes), 8))


def dfree(sess, *ptrs):
    from trino_amd import tpch_queries as tq
    for p in ptrs:
        tq._device_free(sess, p)


def upload(sess, arr):
    from trino_amd import _check
    arr = np.ascontiguousarray(arr)
    p = dbuf(sess, arr.nbytes)
    if arr.nbytes:
        _check(lib().tg_copy_htod(sess._h, p, arr.ctypes.data, arr.nbytes))
    return p


def download(sess, ptr, n, dtype):
    from trino_amd import copy_dtoh
    out = np.empty(n, dtype)
    if n:
        copy_dtoh(sess, out, ptr)
    return out


class VarCol:
    """a device VARCHAR column built by hand: bytes + offsets[n + 1]"""

    def __init__(self, sess, rows):
        self.sess, self.n = sess, len(rows)
        lens = np.fromiter((len(t) for t in rows), np.int64, len(rows))
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        data = np.frombuffer(b"".join(rows), np.uint8)
        self.d_bytes = upload(sess, data)
        self.d_off = upload(sess, offsets)
        self.d_flags = dbuf(sess, self.n)

    def raw(self, pattern, n=None, fill=0xEE):
        """status and the whole flags buffer, pre-filled with `fill`"""
        n = self.n if n is None else n
        pre = np.full(max(self.n, 8), fill, np.uint8)
        from trino_amd import _check
        _check(lib().tg_copy_htod(self.sess._h, self.d_flags, pre.ctypes.data,
                                  pre.nbytes))
        st = lib().tg_varchar_like_flags(self.sess._h, self.d_bytes, self.d_off,
                                         n, pattern, self.d_flags)
        return st, download(self.sess, self.d_flags, max(self.n, 8), np.uint8)

    def flags(self, pattern):
        st, got = self.raw(pattern)
        assert st == TG_OK, (pattern, st)
        return got[:self.n]

    def free(self):
        dfree(self.sess, self.d_bytes, self.d_off, self.d_flags)


def check_like_case(sess, name):
    _, patterns, rows = like_case(name)
    col = VarCol(sess, rows)
    wrong = []
    try:
        for p in patterns:
            exp = np.array([ref_like(p, t) for t in rows], np.uint8)
            assert both_verdicts(exp) or (p in LIKE_ALL_ONE and exp.all()), p
            got = col.flags(p)
            bad = np.flatnonzero(got != exp)
            if bad.size:
                wrong.append((p, bad.size, [(rows[i], int(got[i])) for i in bad[:5]]))
    finally:
        col.free()
    assert not wrong, wrong


# --------------------------------------------------------------------------
# LIKE: tg_varchar_like_flags
# --------------------------------------------------------------------------
def test_like_no_percent_is_equality(sess):
    """L1: a pattern without '%' matches iff the text equals it (the parent
    matched it as a prefix: 'abc' LIKE "abcd")."""
    assert ref_like(b"abc", b"abcd") == 0 and ref_like(b"abc", b"abc") == 1
    check_like_case(sess, "no_percent")


def test_like_empty_pattern(sess):
    """L2: '' matches only the empty text (the parent matched every row)."""
    assert ref_like(b"", b"") == 1 and ref_like(b"", b"a") == 0
    check_like_case(sess, "empty_pattern")


def test_like_anchor_matrix(sess):
    for p, t, v in ANCHOR_BY_HAND:
        assert ref_like(p, t) == v, (p, t)
        assert t in like_case("anchor_matrix")[2]
    check_like_case(sess, "anchor_matrix")


def test_like_swar_lanes(sess):
    """like_find_byte: the word loop, its byte prologue and epilogue, at every
    alignment of the row start, with near-miss bytes in the words before the
    true occurrence."""
    check_like_case(sess, "swar_lanes")


def test_like_bytes_not_chars(sess):
    check_like_case(sess, "bytes_not_chars")


def test_like_limits(sess):
    """4 segments and 63 pattern bytes are accepted; 5 segments, 64 bytes and
    any '_' are TG_ERR_UNSUPPORTED before anything is launched."""
    check_like_case(sess, "limits_accepted")
    _, _, rows = like_case("limits_accepted")
    col = VarCol(sess, rows)
    try:
        for p in LIKE_REJECTED:
            st, buf = col.raw(p)
            assert st == TG_ERR_UNSUPPORTED, (p, st)
            assert (buf == 0xEE).all(), p
    finally:
        col.free()


def test_like_argument_checks(sess):
    """null session / pointer / pattern and n < 0 are TG_ERR_INVALID_ARG and
    leave the flags untouched, on both entry points."""
    L = lib()
    col = VarCol(sess, [b"ab", b"", b"b"])
    d_offs = upload(sess, np.zeros(3, np.int64))
    d_lens = upload(sess, np.ones(3, np.int32))
    try:
        h, by, of, fl = sess._h, col.d_bytes, col.d_off, col.d_flags
        pre = np.full(8, 0xEE, np.uint8)
        from trino_amd import _check
        _check(L.tg_copy_htod(h, fl, pre.ctypes.data, 8))
        for args in ((None, by, of, 3, b"%a%", fl), (h, None, of, 3, b"%a%", fl),
                     (h, by, None, 3, b"%a%", fl), (h, by, of, 3, None, fl),
                     (h, by, of, 3, b"%a%", None), (h, by, of, -1, b"%a%", fl)):
            assert L.tg_varchar_like_flags(*args) == TG_ERR_INVALID_ARG, args
        for args in ((None, d_offs, d_lens, 3, b"%a%", fl),
                     (h, None, d_lens, 3, b"%a%", fl),
                     (h, d_offs, None, 3, b"%a%", fl),
                     (h, d_offs, d_lens, 3, None, fl),
                     (h, d_offs, d_lens, 3, b"%a%", None),
                     (h, d_offs, d_lens, -1, b"%a%", fl),
                     (h, d_offs, d_lens, 3, b"a_", fl)):
            st = L.tg_pool_like_flags(*args)
            assert st == (TG_ERR_UNSUPPORTED if args[4] == b"a_"
                          else TG_ERR_INVALID_ARG), args
        assert (download(sess, fl, 8, np.uint8) == 0xEE).all()
    finally:
        col.free()
        dfree(sess, d_offs, d_lens)


def test_like_grid_stride(sess):
    """more rows than one pass of the grid: the second stride and its tail,
    with a zero-length row first, last and at the seam."""
    rows = like_case("grid_stride")[2]
    assert len(rows) == GRID_N
    assert rows[0] == rows[-1] == rows[GRID_THREADS] == b""
    check_like_case(sess, "grid_stride")


def test_like_zero_rows(sess, monkeypatch):
    col = VarCol(sess, [b"ab", b"b"])
    d_offs = upload(sess, np.zeros(2, np.int64))
    d_lens = upload(sess, np.ones(2, np.int32))
    try:
        for p in (b"%b%", b"ab", b""):
            st, buf = col.raw(p, n=0)
            assert st == TG_OK and (buf == 0xEE).all(), p
            for mode in ("0", "1", "2"):
                monkeypatch.setenv("TG_LIKE_IDX", mode)
                assert lib().tg_pool_like_flags(sess._h, d_offs, d_lens, 0, p,
                                                col.d_flags) == TG_OK
            assert (download(sess, col.d_flags, 8, np.uint8) == 0xEE).all()
    finally:
        col.free()
        dfree(sess, d_offs, d_lens)


# --------------------------------------------------------------------------
# LIKE: tg_pool_like_flags
# --------------------------------------------------------------------------
def pool_flags(sess, d_offs, d_lens, n, pattern, d_flags):
    st = lib().tg_pool_like_flags(sess._h, d_offs, d_lens, n, pattern, d_flags)
    assert st == TG_OK, (pattern, st, lib().tg_last_error())
    return download(sess, d_flags, n, np.uint8)


@pytest.mark.parametrize("mode", ["0", "1", "2"], ids=["mode0", "mode1", "mode2"])
def test_pool_like_constructed_slices(sess, monkeypatch, mode):
    """byte scan / occurrence index / offset-sorted scan over slices cut
    around real occurrences: ending at, one short of, starting at and one
    past an occurrence, empty, and touching both ends of the pool. In mode 1
    the floating patterns and POOL_NOWHERE take the index (four segments,
    eight pool scans in all); the anchored ones fall through to the byte scan."""
    monkeypatch.setenv("TG_LIKE_IDX", mode)
    offs, lens = pool_constructed_slices()
    n = len(offs)
    d_offs, d_lens, d_flags = upload(sess, offs), upload(sess, lens), dbuf(sess, n)
    wrong = []
    try:
        for p in POOL_PATTERNS:
            exp = pool_constructed_expected(p)
            assert both_verdicts(exp) or (p == POOL_NOWHERE and not exp.any()), p
            got = pool_flags(sess, d_offs, d_lens, n, p, d_flags)
            bad = np.flatnonzero(got != exp)
            if bad.size:
                wrong.append((p, mode, bad.size, offs[bad[:5]].tolist(),
                              lens[bad[:5]].tolist()))
    finally:
        dfree(sess, d_offs, d_lens, d_flags)
    assert not wrong, wrong


def test_pool_like_default_switch(sess, monkeypatch):
    """TG_LIKE_IDX unset: 2^20 - 1 rows take the byte scan, 2^20 rows the
    offset-sorted path (k_pack_len_row, the 29-bit pair sort, the scatter by
    row id); rows that share an offset differ in length and in verdict."""
    monkeypatch.delenv("TG_LIKE_IDX", raising=False)
    offs, lens = pool_switch_slices()
    exp = pool_switch_expected()
    n = len(offs)
    assert n == SORTED_SWITCH and both_verdicts(exp)
    d_offs, d_lens, d_flags = upload(sess, offs), upload(sess, lens), dbuf(sess, n)
    try:
        for m in (n - 1, n):
            got = pool_flags(sess, d_offs, d_lens, m, POOL_SWITCH_PATTERN, d_flags)
            bad = np.flatnonzero(got != exp[:m])
            assert bad.size == 0, (m, bad[:5], offs[bad[:5]], lens[bad[:5]])
    finally:
        dfree(sess, d_offs, d_lens, d_flags)


# --------------------------------------------------------------------------
# sorted DISTINCT: tg_dedup_i64
# --------------------------------------------------------------------------
def run_dedup(sess, keys, bits):
    n = len(keys)
    d_in, d_out = upload(sess, keys), dbuf(sess, n * 8)
    try:
        out_n = ctypes.c_int64(-1)
        st = lib().tg_dedup_i64(sess._h, d_in, n, bits, d_out, ctypes.byref(out_n))
        assert st == TG_OK, st
        return out_n.value, download(sess, d_out, max(out_n.value, 0), np.int64)
    finally:
        dfree(sess, d_in, d_out)


@pytest.mark.parametrize("case", [c[0] for c in dedup_cases()])
def test_dedup_edges(sess, ops, case):
    _, keys, bits = next(c for c in dedup_cases() if c[0] == case)
    exp = sorted(set(keys.tolist()))
    m, got = run_dedup(sess, keys, bits)
    assert m == len(exp)
    assert got.tolist() == exp


def test_dedup_key_wider_than_bits(sess, ops):
    """Contract (include/trino_gpu.h): keys must lie in [0, 2^bits). Nothing
    checks it (that would cost a pass over the column); only the low `bits`
    bits order the sort, so the output of wider keys may be unsorted and may
    repeat a key, but it loses none and invents none."""
    keys = np.array([5, 256 + 5, 5, 1, 256 + 1, 512 + 5, 1], np.int64)
    m, got = run_dedup(sess, keys, 8)
    assert set(got.tolist()) == set(keys.tolist())
    assert len(set(keys.tolist())) <= m <= len(keys)


def test_dedup_rejections(sess, ops):
    L = lib()
    d = upload(sess, np.arange(4, dtype=np.int64))
    o = dbuf(sess, 32)
    out_n = ctypes.c_int64(-7)
    ref = ctypes.byref(out_n)
    try:
        for args in ((sess._h, d, 4, 0, o, ref), (sess._h, d, 4, 65, o, ref),
                     (sess._h, d, 4, -1, o, ref), (sess._h, d, -1, 64, o, ref),
                     (None, d, 4, 64, o, ref), (sess._h, None, 4, 64, o, ref),
                     (sess._h, d, 4, 64, None, ref), (sess._h, d, 4, 64, o, None)):
            assert L.tg_dedup_i64(*args) == TG_ERR_INVALID_ARG, args[2:4]
        assert out_n.value == -7
    finally:
        dfree(sess, d, o)


# --------------------------------------------------------------------------
# typed pages (every fixed width, DOUBLE, VARCHAR, validity bitmaps)
# --------------------------------------------------------------------------
T_BIGINT, T_INTEGER, T_SMALLINT, T_TINYINT, T_DOUBLE, T_DATE, T_BOOLEAN, T_VARCHAR = range(8)
NP_OF = {T_BIGINT: np.int64, T_INTEGER: np.int32, T_SMALLINT: np.int16,
         T_TINYINT: np.int8, T_DOUBLE: np.float64, T_DATE: np.int32,
         T_BOOLEAN: np.int8}
FIXED_TYPES = (T_BIGINT, T_INTEGER, T_DATE, T_SMALLINT, T_TINYINT, T_BOOLEAN)


def pack_valid(v):
    n = len(v)
    words = np.zeros(max((n + 63) // 64, 1), np.uint64)
    if n:
        b = np.packbits(np.asarray(v, np.uint8), bitorder="little")
        words.view(np.uint8)[:len(b)] = b
    return words


def unpack_valid(words, n):
    if words is None:
        return np.ones(n, bool)
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8),
                         bitorder="little")
    return bits[:n].astype(bool)


class TCol:
    """one typed channel on the host. Fixed width: `values` a numpy array of
    NP_OF[tg]; VARCHAR: `values` a list of bytes. valid: bool array or None.
    A NULL cell keeps whatever data word / bytes the caller put under it."""

    def __init__(self, tg, values, valid=None):
        self.tg = tg
        self.valid = None if valid is None else np.asarray(valid, bool)
        if tg == T_VARCHAR:
            self.values = list(values)
        else:
            self.values = np.ascontiguousarray(values, NP_OF[tg])

    def __len__(self):
        return len(self.values)

    def cut(self, lo, hi):
        return TCol(self.tg, self.values[lo:hi],
                    None if self.valid is None else self.valid[lo:hi])

    def cells(self):
        """Python cells, None for NULL"""
        v = self.values if self.tg == T_VARCHAR else self.values.tolist()
        if self.valid is None:
            return list(v)
        return [x if o else None for x, o in zip(v, self.valid.tolist())]


def typed_page(ops, cols):
    entries, valids = [], []
    for c in cols:
        if c.tg == T_VARCHAR:
            lens = [len(t) for t in c.values]
            offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            data = np.frombuffer(b"".join(c.values) or b"\0", np.uint8).copy()
            entries.append((data, offsets))
        else:
            entries.append(c.values)
        valids.append(None if c.valid is None else pack_valid(c.valid))
    page = ops.page_with_varchar(entries, valids)
    for i, c in enumerate(cols):
        page.blocks[i].type = c.tg
    return page


def assert_channel_unchanged(pages_out, ch, pages_in):
    """output channel `ch` of every page == the input channel, byte for byte
    (data words under NULL cells included), type and validity bits too"""
    assert len(pages_out) == len(pages_in)
    for po, pi in zip(pages_out, pages_in):
        src, got = pi[ch], po[ch]
        n = len(src)
        assert got["type"] == src.tg
        assert len(got["values"]) == n
        if src.tg == T_VARCHAR:
            assert list(got["values"]) == src.values
        else:
            assert np.array_equal(np.asarray(got["values"]).view(np.uint8),
                                  src.values.view(np.uint8))
        if src.valid is None:
            assert got["valid"] is None
        else:
            assert got["valid"] is not None
            assert np.array_equal(unpack_valid(got["valid"], n), src.valid)


# --------------------------------------------------------------------------
# MarkDistinct
# --------------------------------------------------------------------------
def run_mark(sess, ops, key_chs, pages):
    """pages: list of TCol lists. Returns the downloaded output pages."""
    tys = [pages[0][c].tg for c in key_chs]
    op = ops.mark_distinct(sess, key_chs, tys)
    try:
        for p in pages:
            op.add_input(typed_page(ops, p))
        return op.drain()
    finally:
        op.close()


def check_mark(sess, ops, key_chs, pages):
    out = run_mark(sess, ops, key_chs, pages)
    nch = len(pages[0])
    rows = []
    for p in pages:
        rows += list(zip(*[p[c].cells() for c in key_chs])) if key_chs else \
            [()] * len(p[0])
    exp = np.array(ref_mark_distinct(rows), np.int8)
    assert len(out) == len(pages)
    for po in out:
        assert len(po) == nch + 1
        assert po[nch]["type"] == T_BOOLEAN and po[nch]["valid"] is None
    got = np.concatenate([np.asarray(po[nch]["values"]) for po in out])
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (bad[:8], got[bad[:8]], [rows[i] for i in bad[:8]])
    for ch in range(nch):
        assert_channel_unchanged(out, ch, pages)
    return exp


NAN_PAYLOADS = (0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000123)


def double_key_values(n, seed):
    r = np.random.default_rng(seed)
    special = np.array([0.0, -0.0, math.inf, -math.inf, 1.5, -1.5, 2.0 ** -1074])
    v = special[r.integers(0, len(special), n)].copy()
    nan_at = r.random(n) < 0.2
    bits = v.view(np.uint64)
    bits[nan_at] = np.array(NAN_PAYLOADS, np.uint64)[r.integers(0, 3, int(nan_at.sum()))]
    v[:7] = special
    v.view(np.uint64)[7:10] = np.array(NAN_PAYLOADS, np.uint64)
    return v


def varchar_key_values(n, seed):
    r = random.Random(seed)
    pool = [b"", b"a", b"ab", b"abc", b"abd", b"ba", b"\x00", b"\x00\x00",
            b"abcdefgh", b"abcdefgi", b"abcdefghi", b"\xc3\xa9", b"A"]
    return pool + [r.choice(pool) for _ in range(n - len(pool))]


def mark_key_column(kind, n, with_valid, seed):
    r = np.random.default_rng(seed)
    if kind == T_DOUBLE:
        vals = double_key_values(n, seed)
    elif kind == T_VARCHAR:
        vals = varchar_key_values(n, seed)
    elif kind == T_BOOLEAN:
        vals = r.integers(0, 2, n)
    else:
        info = np.iinfo(NP_OF[kind])
        near = np.array([info.min, info.min + 1, -1, 0, 1, info.max - 1, info.max])
        vals = near[r.integers(0, len(near), n)]
    valid = None
    if with_valid:
        valid = r.random(n) >= 0.25
        valid[:14] = True                 # the named special values stay keys
        valid[14] = False
    return TCol(kind, vals, valid)


MARK_N = 3001


@functools.lru_cache(None)
def mark_key_type_case(kind, with_valid):
    key = mark_key_column(kind, MARK_N, with_valid, 100 + kind)
    other = TCol(T_BIGINT, np.arange(MARK_N, dtype=np.int64) * 7)
    return [[other.cut(0, 1200), key.cut(0, 1200)],
            [other.cut(1200, MARK_N), key.cut(1200, MARK_N)]]


@pytest.mark.parametrize("with_valid", [False, True], ids=["dense", "bitmap"])
@pytest.mark.parametrize("kind", FIXED_TYPES + (T_DOUBLE, T_VARCHAR),
                         ids=["bigint", "integer", "date", "smallint", "tinyint",
                              "boolean", "double", "varchar"])
def test_mark_key_types(sess, ops, kind, with_valid):
    """one key channel of each type, extreme values of its width; DOUBLE with
    -0.0/0.0, three NaN payloads (one with the sign bit) and +-inf; VARCHAR
    with b'', a NULL cell, shared prefixes and equal lengths."""
    pages = mark_key_type_case(kind, with_valid)
    exp = check_mark(sess, ops, [1], pages)
    assert 1 < int(exp.sum()) < len(exp)


@functools.lru_cache(None)
def mark_multi_case(nch):
    """nch key channels over two values each, every cell NULL with
    probability 1/3: (NULL, 1), (NULL, 2), (NULL, NULL) ... all occur"""
    n = 4001
    r = np.random.default_rng(200 + nch)
    kinds = (T_BIGINT, T_INTEGER, T_DOUBLE, T_SMALLINT, T_VARCHAR, T_TINYINT,
             T_DATE)[:nch]
    cols = []
    for k in kinds:
        pick = r.integers(0, 2, n)
        if k == T_VARCHAR:
            vals = [(b"x", b"")[i] for i in pick.tolist()]
        elif k == T_DOUBLE:
            vals = np.where(pick == 1, -0.0, math.nan)
        else:
            vals = pick + 1
        cols.append(TCol(k, vals, r.integers(0, 3, n) != 0))
    cols.append(TCol(T_DOUBLE, r.standard_normal(n)))
    return [[c.cut(0, 1500) for c in cols], [c.cut(1500, n) for c in cols]]


@pytest.mark.parametrize("nch", [2, 4, 7])
def test_mark_multi_channel_nulls(sess, ops, nch):
    """NULL is a key value in every position; 7 channels take the dynamic
    k_gt_assign<0> kernel."""
    pages = mark_multi_case(nch)
    rows = set()
    for p in pages:
        rows |= set(zip(*[p[c].cells() for c in range(nch)]))
    for pos in range(nch):
        assert any(r[pos] is None for r in rows)
    assert any(all(v is None for v in r) for r in rows)
    check_mark(sess, ops, list(range(nch)), pages)


def test_mark_hot_key(sess, ops):
    """200,000 rows of one key: every thread races on one first_row cell;
    exactly row 0 is flagged, and a second page of the key carries no flag."""
    n = 200_000
    key = TCol(T_BIGINT, np.full(n, -42, np.int64))
    exp = check_mark(sess, ops, [0], [[key], [key.cut(0, 1000)]])
    assert exp[0] == 1 and int(exp.sum()) == 1


GROWTH_NEW, GROWTH_REPEAT = 40_000, 100


@functools.lru_cache(None)
def mark_growth_pages():
    pages = []
    for p in range(3):
        new = np.arange(GROWTH_NEW, dtype=np.int64) * 3 + p * 10 ** 9
        rep = np.arange(GROWTH_REPEAT, dtype=np.int64) * 3 * 17    # keys of page 1
        keys = np.concatenate([new[:20_000], rep, new[20_000:]])
        pages.append([TCol(T_BIGINT, keys)])
    return pages


def test_mark_across_growth(sess, ops):
    """three pages of 40,000 new keys (+100 repeats of page-1 keys): page 2
    grows the key store past 65,536 groups with live first_row, page 3 grows
    the slot table (rehash). Repeats stay unflagged, new keys flag once."""
    pages = mark_growth_pages()
    exp = check_mark(sess, ops, [0], pages)
    per = GROWTH_NEW + GROWTH_REPEAT
    assert int(exp[:per].sum()) == GROWTH_NEW          # page 1 repeats itself
    assert int(exp[per:].sum()) == 2 * GROWTH_NEW


def test_mark_page_edges(sess, ops):
    """zero-row pages first, in the middle and last; a one-row page; a
    duplicate straddling a page boundary; VARCHAR key next to the empty pages
    (contract: accepted)."""
    def page(ks, vs):
        return [TCol(T_BIGINT, np.array(ks, np.int64)), TCol(T_VARCHAR, vs)]
    pages = [page([], []), page([5, 6, 7], [b"a", b"", b"a"]), page([], []),
             page([7], [b"a"]), page([7, 5, 8], [b"b", b"a", b""]), page([], [])]
    exp = check_mark(sess, ops, [0, 1], pages)
    assert exp.tolist() == [1, 1, 1, 0, 1, 0, 1]
    check_mark(sess, ops, [1], pages)
    check_mark(sess, ops, [0], pages)


def test_mark_grid_stride(sess, ops):
    """524,545 rows in one page: the second grid stride of k_gt_assign and
    k_mark_first (and a key store grown 16-fold before the page runs)."""
    r = np.random.default_rng(9)
    keys = r.integers(0, 300_000, GRID_N).astype(np.int64)
    keys[GRID_THREADS:] = keys[:257]                   # the tail repeats row 0..256
    exp = check_mark(sess, ops, [0], [[TCol(T_BIGINT, keys)]])
    assert int(exp[GRID_THREADS:].sum()) == 0


def test_mark_no_key_channels(sess, ops):
    """zero key channels: one global group; only global row 0 is flagged"""
    def page(n, base):
        return [TCol(T_INTEGER, np.arange(n, dtype=np.int32) + base)]
    exp = check_mark(sess, ops, [], [page(70, 0), page(1, 70), page(130, 71)])
    assert exp[0] == 1 and int(exp.sum()) == 1


def test_mark_passthrough_columns(sess, ops):
    """non-key channels of every width plus VARCHAR, with bitmaps, come out
    unchanged (check_mark compares every channel byte for byte); the flag
    channel is BOOLEAN without a bitmap, i.e. valid everywhere."""
    n = 1000
    r = np.random.default_rng(31)
    cols = [TCol(T_INTEGER, r.integers(0, 50, n))]
    for k in FIXED_TYPES + (T_DOUBLE, T_VARCHAR):
        c = mark_key_column(k, n, True, 300 + k)
        cols.append(c)
        cols.append(TCol(k, c.values))                 # and without a bitmap
    pages = [[c.cut(0, 129) for c in cols], [c.cut(129, n) for c in cols]]
    check_mark(sess, ops, [0], pages)


# --------------------------------------------------------------------------
# adaptive partial aggregation: pass-through
# --------------------------------------------------------------------------
PARTIAL, FINAL, SINGLE = 0, 1, 2
SP_GRID, SP_MONEY = 10, 43
TWO_WORD = (FN_AVG_F64, FN_SUM_F64_EXACT)


def amx():
    import test_gpu_aggregation_matrix as m
    return m


PA_MAX_PARTIAL = 1 << 20     # re-enables after 1.5 * 200 * 2^20 = 300 MiB of input,
                             # more than any test here passes through


def flip(ctrl):
    """another driver of the plan node flips it: a synthetic flush of 2 MiB
    (>= 1.5 * PA_MAX_PARTIAL) in which every row was unique"""
    ctrl.on_flush(2 * PA_MAX_PARTIAL, 100, 100, True)
    assert ctrl.disabled


def disabled_controller(ops):
    ctrl = ops.PartialAggController(max_partial_bytes=PA_MAX_PARTIAL, threshold=0.8)
    flip(ctrl)
    return ctrl


def pa_aggs(base):
    """every aggregate function over [iv, fv, em] at channels base.."""
    A = amx().Agg
    return [A(FN_COUNT_STAR), A(FN_COUNT_COL, base), A(FN_SUM_F64, base + 1),
            A(FN_SUM_I64, base), A(FN_AVG_F64, base + 1),
            A(FN_SUM_F64_EXACT, base + 1, SP_GRID), A(FN_MIN_I64, base),
            A(FN_MAX_I64, base), A(FN_SUM_F64_EXACT, base + 2, SP_MONEY)]


def pa_value_cols(n, seed, null_rate=0.4):
    """[iv BIGINT, fv DOUBLE on the 2^-10 grid below 2^30 (both signs), em
    money grid], each ~40 % NULL with a hostile word under every NULL cell.
    Sums of fewer than 2^13 such fv cells are exact in f64 in any order."""
    m = amx()
    r = np.random.default_rng(seed)
    iv = r.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    fv = r.integers(-2 ** 40 + 1, 2 ** 40, n).astype(np.float64) / 1024.0
    em = r.integers(90100, 209900, n).astype(np.float64) / 100.0
    cols = []
    for v, poison in ((iv, m.POISON_I), (fv, math.nan), (em, math.nan)):
        ok = r.random(n) >= null_rate
        v = v.copy()
        v[~ok] = poison
        cols.append(m.Col(v, ok))
    return cols


def all_null(col):
    m = amx()
    v = col.values.copy()
    v[:] = m.POISON_I if v.dtype == np.int64 else math.nan
    return m.Col(v, np.zeros(len(v), bool))


def concat_cols(parts):
    m = amx()
    out = []
    for cs in zip(*parts):
        valid = None
        if any(c.valid is not None for c in cs):
            valid = np.concatenate([c.ok() for c in cs])
        out.append(m.Col(np.concatenate([c.values for c in cs]), valid))
    return out


def col_cells(col):
    v = col.values.tolist()
    return v if col.valid is None else [x if o else None
                                        for x, o in zip(v, col.valid.tolist())]


def assert_states(out_pages, in_pages, nk, aggs):
    """the pass-through pages: one row per input row, keys unchanged, every
    state channel == ref_partial_state bit for bit and without a bitmap"""
    assert len(out_pages) == len(in_pages)
    for po, cols in zip(out_pages, in_pages):
        n = len(cols[0].values)
        ch = nk
        for ag in aggs:
            cells = [None] * n if ag.fn == FN_COUNT_STAR else col_cells(cols[ag.ch])
            exp = [ref_partial_state(ag.fn, c, ag.scale_pow) for c in cells]
            for w in range(2 if ag.fn in TWO_WORD else 1):
                blk = po[ch]
                is_f64 = (ag.fn == FN_SUM_F64) or (ag.fn == FN_AVG_F64 and w == 1)
                assert blk["type"] == (T_DOUBLE if is_f64 else T_BIGINT), (ag.fn, w)
                assert blk["valid"] is None
                got = np.asarray(blk["values"]).view(np.int64)
                e = np.array([x[w] for x in exp], np.int64)
                assert len(got) == n
                bad = np.flatnonzero(got != e)
                assert bad.size == 0, (ag.fn, w, bad[:5], got[bad[:5]], e[bad[:5]])
                ch += 1
        assert ch == len(po)


def pages_to_cols(pages):
    """downloaded pages -> one Col list (to feed a FINAL operator)"""
    m = amx()
    out = []
    for c in range(len(pages[0])):
        vals = np.concatenate([np.asarray(p[c]["values"]) for p in pages])
        valid = np.concatenate([unpack_valid(p[c]["valid"], len(p[c]["values"]))
                                for p in pages])
        out.append(m.Col(vals, None if valid.all() else valid))
    return out


def run_final(sess, ops, pcols, key_chs, key_tys, aggs, cuts=()):
    m = amx()
    op = ops.hash_aggregation(sess, key_chs, key_tys,
                              [a.spec() for a in m.final_aggs(aggs, len(key_chs))],
                              step=FINAL)
    m.feed(op, ops, pcols, cuts)
    return m.collect(op)


def check_bit_exact(ref, out, nk, aggs):
    """FINAL output == the SINGLE reference, group for group (matched by key,
    the FINAL sees the keys in another order), every kind bit for bit. The
    one recorded deviation: a SUM over no non-NULL input is 0, not NULL."""
    assert out is not None and len(out) == nk + len(aggs)
    ng = len(ref.keys)
    assert all(len(v) == ng for v, _ in out)
    keys = list(zip(*[[x if o else None for x, o in zip(v.tolist(), ok.tolist())]
                      for v, ok in out[:nk]])) if nk else [()]
    assert len(set(keys)) == ng and set(keys) == set(ref.keys)
    row = {k: i for i, k in enumerate(keys)}
    perm = np.array([row[k] for k in ref.keys])
    for a, ag in enumerate(aggs):
        got, gvalid = out[nk + a]
        got, gvalid = got[perm], gvalid[perm]
        for g, e in enumerate(ref.cols[a]):
            if e is None and ag.fn in (FN_SUM_F64, FN_SUM_I64, FN_SUM_F64_EXACT):
                assert gvalid[g] and got[g] == 0, (ag.fn, g)
            elif e is None:
                assert not gvalid[g], (ag.fn, g)
            else:
                assert gvalid[g], (ag.fn, g)
                if isinstance(e, float):
                    assert f64_bits(float(got[g])) == f64_bits(e), (ag.fn, g, got[g], e)
                else:
                    assert int(got[g]) == e, (ag.fn, g, got[g], e)


def test_pa_state_every_aggregate_with_nulls(sess, ops):
    """every aggregate in one pass-through operator, ~40 % NULL inputs plus
    an all-NULL page and a group (key 3) whose cells are NULL everywhere."""
    m = amx()
    n = 1000
    gid = np.arange(n, dtype=np.int64) % 7
    p1 = [m.Col(gid * 11)] + pa_value_cols(n, 501)
    for c in p1[1:]:
        c.valid = c.valid & (gid != 3)
        c.values[gid == 3] = m.POISON_I if c.values.dtype == np.int64 else math.nan
    p2 = [m.Col(gid[:130] * 11)] + [all_null(c) for c in pa_value_cols(130, 502)]
    aggs = pa_aggs(1)
    ctrl = disabled_controller(ops)
    op = ops.hash_aggregation(sess, [0], [ops.TG_BIGINT], [a.spec() for a in aggs],
                              step=PARTIAL)
    ctrl.attach(op)
    for p in (p1, p2):
        op.add_input(m.make_page(ops, p, 0, len(p[0].values)))
    out = op.drain()
    op.close()
    ctrl.close()
    assert_states(out, [p1, p2], 1, aggs)
    for po, p in zip(out, (p1, p2)):
        assert np.array_equal(po[0]["values"], p[0].values) and po[0]["valid"] is None
    allc = concat_cols([p1, p2])
    ref = m.reference(allc, [0], aggs)
    g3 = ref.keys.index((33,))
    assert [c[g3] for c in ref.cols] == [143 + 19, 0, None, None, None, None,
                                         None, None, None]
    fin = run_final(sess, ops, pages_to_cols(out), [0], [ops.TG_BIGINT], aggs, (700,))
    check_bit_exact(ref, fin, 1, aggs)


PA_KEY_FORMS = tuple((k,) for k in FIXED_TYPES + (T_DOUBLE,)) + (
    (T_BIGINT, T_INTEGER), (T_SMALLINT, T_DOUBLE, T_DATE))
PA_BITMAP_NS = (63, 64, 65, 129)


@pytest.mark.parametrize("n", PA_BITMAP_NS)
@pytest.mark.parametrize("form", PA_KEY_FORMS, ids=lambda f: "-".join(map(str, f)))
def test_pa_group_key_widths_and_bitmaps(sess, ops, form, n):
    """pass-through copies group keys of every fixed width and DOUBLE, one to
    three channels, with their validity bitmaps (the word-count copy at
    n = 63, 64, 65, 129) unchanged, in group-channel order."""
    nk = len(form)
    keys = [mark_key_column(k, max(n, 15), True, 700 + 10 * i + k).cut(0, n)
            for i, k in enumerate(form)]
    keys[-1].valid[n - 1] = False                       # the last bit of the bitmap
    keys[0].valid[n - 1] = True
    val = TCol(T_BIGINT, np.arange(n, dtype=np.int64) - 5)
    cols = [val] + keys                                  # keys at channels 1..nk
    key_chs = list(range(nk, 0, -1))                     # and named in reverse
    ctrl = disabled_controller(ops)
    op = ops.hash_aggregation(sess, key_chs, [cols[c].tg for c in key_chs],
                              [(FN_COUNT_STAR, -1), (FN_SUM_I64, 0)], step=PARTIAL)
    ctrl.attach(op)
    op.add_input(typed_page(ops, cols))
    out = op.drain()
    op.close()
    ctrl.close()
    assert len(out) == 1 and len(out[0]) == nk + 2
    for i, c in enumerate(key_chs):
        assert_channel_unchanged([[out[0][i]]], 0, [[cols[c]]])
    assert np.array_equal(out[0][nk]["values"], np.ones(n, np.int64))
    assert np.array_equal(out[0][nk + 1]["values"], val.values)


def test_pa_mixed_partials_equal_single(sess, ops):
    """page 1 aggregated (controller enabled), pages 2 and 3 passed through
    by the same operator after the controller flips, page 4 aggregated by a
    second operator on a fresh controller: FINAL over all partial pages ==
    the SINGLE reference over all the input. Every kind bit for bit: the f64
    inputs lie on the 2^-10 grid below 2^30 and every group has fewer than
    2^13 rows, so each partial sum is exact and the order cannot matter."""
    m = amx()
    n, cuts = 2200, (0, 500, 1100, 1700, 2200)
    r = np.random.default_rng(601)
    kv = r.integers(0, 40, n).astype(np.int64) * 1001 - 7
    kok = r.random(n) >= 0.05                            # a NULL-key group too
    kv[~kok] = m.POISON_I
    cols = [m.Col(kv, kok)] + pa_value_cols(n, 602)
    aggs = pa_aggs(1)
    specs = [a.spec() for a in aggs]
    pages = [[m.Col(c.values[a:b], c.ok()[a:b]) for c in cols]
             for a, b in zip(cuts[:-1], cuts[1:])]

    def page(i):
        return m.make_page(ops, pages[i], 0, len(pages[i][0].values))

    ctrl = ops.PartialAggController(max_partial_bytes=PA_MAX_PARTIAL, threshold=0.8)
    op1 = ops.hash_aggregation(sess, [0], [ops.TG_BIGINT], specs, step=PARTIAL)
    ctrl.attach(op1)
    assert not ctrl.disabled
    op1.add_input(page(0))
    flip(ctrl)
    op1.add_input(page(1))
    op1.add_input(page(2))
    out1 = op1.drain()
    op1.close()
    ctrl.close()
    through = [p for p in out1 if len(p[0]["values"]) in (600,)]
    assert len(out1) == 3 and len(through) == 2
    assert_states(through, [pages[1], pages[2]], 1, aggs)
    ctrl2 = ops.PartialAggController(max_partial_bytes=1 << 30, threshold=0.8)
    op2 = ops.hash_aggregation(sess, [0], [ops.TG_BIGINT], specs, step=PARTIAL)
    ctrl2.attach(op2)
    op2.add_input(page(3))
    out2 = op2.drain()
    op2.close()
    assert not ctrl2.disabled
    ctrl2.close()
    assert len(out2) == 1 and len(out2[0][0]["values"]) <= 41
    ref = m.reference(cols, [0], aggs)
    assert (None,) in ref.keys and max(ref.sizes) < 2 ** 13
    fin = run_final(sess, ops, pages_to_cols(out1 + out2), [0], [ops.TG_BIGINT],
                    aggs, (333, 1000))
    check_bit_exact(ref, fin, 1, aggs)


PA_STRIDE_SP = 10


@functools.lru_cache(None)
def pa_stride_case():
    """524,545 rows, no group channels: [iv, fv on the 2^-10 grid below 2^20]
    (the scalar sum of all of them stays below 2^53 grid steps: exact)"""
    m = amx()
    r = np.random.default_rng(603)
    n = GRID_N
    iv = r.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    fv = r.integers(-2 ** 30 + 1, 2 ** 30, n).astype(np.float64) / 1024.0
    cols = []
    for v, poison in ((iv, m.POISON_I), (fv, math.nan)):
        ok = r.random(n) >= 0.4
        ok[[0, GRID_THREADS - 1, GRID_THREADS, n - 1]] = [True, False, True, False]
        v[~ok] = poison
        cols.append(m.Col(v, ok))
    A = m.Agg
    aggs = [A(FN_COUNT_COL, 0), A(FN_SUM_F64_EXACT, 1, PA_STRIDE_SP), A(FN_MIN_I64, 0)]
    return cols, aggs, m.reference(cols, [], aggs)


def test_pa_scalar_and_edges(sess, ops):
    """no group channels; a zero-row page (before and after); 524,545 rows
    for the second grid stride of k_pa_state."""
    m = amx()
    cols, aggs, ref = pa_stride_case()
    empty = [m.Col(c.values[:0], c.ok()[:0]) for c in cols]
    ctrl = disabled_controller(ops)
    op = ops.hash_aggregation(sess, [], [], [a.spec() for a in aggs], step=PARTIAL)
    ctrl.attach(op)
    ins = [empty, cols, empty]
    for p in ins:
        op.add_input(m.make_page(ops, p, 0, len(p[0].values)))
    out = op.drain()
    op.close()
    assert ctrl.disabled                       # 8 MiB passed: far from re-enabling
    ctrl.close()
    through = out[:3]                          # then the idle table's empty page
    assert [len(p[0]["values"]) for p in out] == [0, GRID_N, 0] + [0] * (len(out) - 3)
    assert_states(through, ins, 0, aggs)
    fin = run_final(sess, ops, pages_to_cols(out), [], [], aggs, (GRID_THREADS,))
    check_bit_exact(ref, fin, 0, aggs)
