"""Join parity matrix: hash build, lookup join (inner and probe-outer), semi
join and set builder against an exact reference written here (no oracle, no
trino_amd join), at the build and probe sizes where each kernel of
trino_amd/csrc/ops_join.hip takes another path.

Reference: ref_join(build_keys, probe_keys, outer) over per-row Python key
tuples (None = NULL component) returns (probe_row, build_row | None) pairs:
probe rows ascending, the matching build rows of one probe row DESCENDING
(reverse insertion, ArrayPositionLinks), a key with a NULL component never
matches, and with `outer` an unmatched probe row emits one (i, None).
Equality is SQL `=`: integers by value, VARCHAR by bytes, DOUBLE by IEEE ==
(-0.0 matches 0.0; NaN matches nothing, itself included). ref_semi gives
True / False / None per probe row by three-valued IN: a hit is True, a NULL
probe is False against a build of zero rows and NULL otherwise, a miss
against a build that contains a NULL key is NULL. ref_join_vec is the
vectorised twin for single BIGINT keys (stable argsort + searchsorted) used
at 2^20 build rows.

Comparison: bit-exact and in list order, no tolerances anywhere: the output
row count, every gathered probe and build column (fixed-width values;
VARCHAR bytes and offsets, a NULL cell having zero length) and every validity
bitmap wherever the reference says NULL or not NULL. The data word under
every NULL input cell holds a poison value: a build NULL key carries a key
the probe asks for, other NULL cells a constant no valid cell holds. Under
TG_JOIN_CSR=0 only (legacy chains, ordered for single-workgroup builds only)
the pairs of one probe row are compared as a set.

Every build and probe page carries its global row number as a BIGINT column,
so the (probe_row, build_row) pairs are read straight off the output.

The host-side checks of this reference and of the shape constructors live in
tests/test_oracle_units.py (they need no GPU).
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "trino_amd", "csrc")


# --------------------------------------------------------------------------
# constants of the code under test, parsed from its sources
# --------------------------------------------------------------------------
@functools.lru_cache(None)
def source_constants():
    """JREG_SLOTS, JSCAN_CHUNK, TG_BLOCK, TG_MAX_BLOCKS, the load-factor
    table of join_hash_size and the murmur3 finalizer constants"""
    join = open(os.path.join(_CSRC, "ops_join.hip")).read()
    common = open(os.path.join(_CSRC, "common.h")).read()
    dev = open(os.path.join(_CSRC, "dev_hash.h")).read()

    def one(pat, text):
        m = re.search(pat, text)
        assert m, pat
        return m

    lf = one(r"expected <= \(1 << (\d+)\) \? ([\d.]+) : expected <= \(1 << (\d+)\) "
             r"\? ([\d.]+) : ([\d.]+);", join)
    mm = one(r"d_murmur3_mix\(uint64_t h\)\s*\{\s*h \^= h >> 33; h \*= 0x([0-9A-Fa-f]+)ULL;"
             r"\s*h \^= h >> 33; h \*= 0x([0-9A-Fa-f]+)ULL;\s*h \^= h >> 33;", dev)
    return dict(
        JREG_SLOTS=int(one(r"#define JREG_SLOTS (\d+)", join).group(1)),
        JSCAN_CHUNK=int(one(r"#define JSCAN_CHUNK (\d+)", join).group(1)),
        TG_BLOCK=int(one(r"constexpr int TG_BLOCK = (\d+);", common).group(1)),
        TG_MAX_BLOCKS=int(one(r"constexpr int TG_MAX_BLOCKS = (\d+);", common).group(1)),
        LOAD=((1 << int(lf.group(1)), float(lf.group(2))),
              (1 << int(lf.group(3)), float(lf.group(4))),
              (None, float(lf.group(5)))),
        MIX=(int(mm.group(1), 16), int(mm.group(2), 16)),
        PART_BYTES=int(one(r"tbl_bytes / nparts > \((\d+)ll << 20\)", join).group(1)) << 20,
    )


def join_hash_size(expected):
    """join_hash_size of ops_join.hip restated over the parsed table"""
    f = next(f for lim, f in source_constants()["LOAD"]
             if lim is None or expected <= lim)
    need = max(int(expected / f), 2)
    cap = 1
    while cap < need:
        cap <<= 1
    return cap


def murmur3_mix(h):
    """d_murmur3_mix over a uint64 numpy array"""
    c1, c2 = (np.uint64(c) for c in source_constants()["MIX"])
    h = np.asarray(h).astype(np.uint64)
    s = np.uint64(33)
    h = (h ^ (h >> s)) * c1
    h = (h ^ (h >> s)) * c2
    return h ^ (h >> s)


def slots_of(keys, capacity):
    return (murmur3_mix(np.asarray(keys, np.int64).view(np.uint64))
            & np.uint64(capacity - 1)).astype(np.int64)


WAVE = 64
JREG_SLOTS = 32768
JSCAN_CHUNK = 65536
GRID_THREADS = 2048 * 256          # tg_grid_for cap: blocks x block size
SMALL_BUILDS = (0, 1, 2, 63, 64, 65, 1000)
REGION_BUILDS = (8192, 8193)       # capacity 32768 = 1 region | 65536 = 2
LOAD_BUILDS = (65536, 65537)       # load factor 0.25 | 0.50
BIG_BUILD = 1 << 20                # capacity 2^21, 64 regions, 2 partitions
PROBE_EDGES = (1, 63, 64, 65, JSCAN_CHUNK - 1, JSCAN_CHUNK, JSCAN_CHUNK + 1,
               2 * JSCAN_CHUNK + 1)
GRID_STRIDE_M = GRID_THREADS + 197  # second stride, partial last wave
SMALL_M = 257
OVERFLOW_N = 64                    # 64 x 64 matches against cap 64 + 64 + 64

POISON_I = 2 ** 62 + 12345         # data word under a NULL integer cell
POISON_S = b"<poison under NULL>"

CSR = os.environ.get("TG_JOIN_CSR", "1") != "0"   # read once, like the library
ORDER = "list" if CSR else "set"

TG_ERR_INVALID_ARG, TG_ERR_UNSUPPORTED = 1, 6


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


@pytest.fixture
def partitioned():
    """route every eligible probe through the partitioned path"""
    names = {"TG_JOIN_PART": "1", "TG_JOIN_PART_MIN_ROWS": "0",
             "TG_JOIN_PART_MIN_BYTES": "0"}
    old = {k: os.environ.get(k) for k in names}
    os.environ.update(names)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def rng(seed=0):
    return np.random.default_rng(seed)


# --------------------------------------------------------------------------
# reference
# --------------------------------------------------------------------------
def _has_null(key):
    return any(c is None for c in key)


def _unmatchable(key):
    return any(c is None or (isinstance(c, float) and c != c) for c in key)


def ref_join(build_keys, probe_keys, outer):
    index = {}
    for r, k in enumerate(build_keys):
        if not _unmatchable(k):
            index.setdefault(k, []).append(r)    # -0.0 == 0.0 and hash alike
    out = []
    for i, k in enumerate(probe_keys):
        rows = () if _unmatchable(k) else index.get(k, ())
        out.extend((i, r) for r in reversed(rows))
        if outer and not rows:
            out.append((i, None))
    return out


def ref_semi(build_keys, probe_keys):
    build_has_null = any(_has_null(k) for k in build_keys)
    present = {k for k in build_keys if not _unmatchable(k)}
    out = []
    for k in probe_keys:
        if _has_null(k):
            out.append(None if len(build_keys) else False)
        elif not _unmatchable(k) and k in present:
            out.append(True)
        else:
            out.append(None if build_has_null else False)
    return out


def ref_join_vec(bk, bvalid, pk, pvalid):
    """inner-join twin of ref_join for single BIGINT keys: (probe_rows,
    build_rows) as int64 arrays; bvalid / pvalid are bool arrays or None"""
    bk, pk = np.asarray(bk, np.int64), np.asarray(pk, np.int64)
    rows = np.arange(len(bk)) if bvalid is None else np.flatnonzero(bvalid)
    order = rows[np.argsort(bk[rows], kind="stable")]   # equal keys: rows ascending
    sk = bk[order]
    lo = np.searchsorted(sk, pk, "left")
    hi = np.searchsorted(sk, pk, "right")
    cnt = hi - lo
    if pvalid is not None:
        cnt = np.where(pvalid, cnt, 0)
    total = int(cnt.sum())
    op = np.repeat(np.arange(len(pk), dtype=np.int64), cnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ob = order[np.repeat(hi, cnt) - 1 - within] if total else np.empty(0, np.int64)
    return op, ob.astype(np.int64)


def ref_semi_vec(bk, bvalid, pk, pvalid):
    """ref_semi twin for single BIGINT keys: (match bool, is_null bool)"""
    bk, pk = np.asarray(bk, np.int64), np.asarray(pk, np.int64)
    bv = np.ones(len(bk), bool) if bvalid is None else bvalid
    pv = np.ones(len(pk), bool) if pvalid is None else pvalid
    hit = np.isin(pk, bk[bv]) & pv
    build_has_null = not bv.all()
    null = (~pv & (len(bk) > 0)) | (pv & ~hit & build_has_null)
    return hit, null


# --------------------------------------------------------------------------
# columns and pages
# --------------------------------------------------------------------------
_NP = {"i64": np.int64, "i32": np.int32, "i16": np.int16, "i8": np.int8,
       "f64": np.float64, "date": np.int32}


class Col:
    """one column: kind, values (numpy array, or list of bytes for 'str') and
    valid (bool array, or None = the page carries no bitmap)"""

    def __init__(self, kind, values, valid=None):
        self.kind = kind
        if kind == "str":
            self.values = list(values)
        else:
            self.values = np.ascontiguousarray(values, _NP[kind])
        self.valid = None if valid is None else np.asarray(valid, bool)
        assert self.valid is None or len(self.valid) == len(self.values)

    def __len__(self):
        return len(self.values)

    def slice(self, lo, hi, keep_bitmap):
        v = None if (self.valid is None or not keep_bitmap) else self.valid[lo:hi]
        if not keep_bitmap and self.valid is not None:
            assert self.valid[lo:hi].all(), "a NULL in a page without a bitmap"
        return Col(self.kind, self.values[lo:hi], v)

    def cell(self, i):
        """Python value of row i, None for NULL"""
        if self.valid is not None and not self.valid[i]:
            return None
        v = self.values[i]
        if self.kind == "str":
            return bytes(v)
        return float(v) if self.kind == "f64" else int(v)


def nullable(kind, values, null_mask, poison=None):
    """column with NULLs where null_mask is set and `poison` under them
    (None: the cell keeps its value, which would match if it were read)"""
    null_mask = np.asarray(null_mask, bool)
    if kind == "str":
        vals = [v if (poison is None or not z) else poison
                for v, z in zip(values, null_mask)]
    else:
        vals = np.array(values, _NP[kind])
        if poison is not None:
            vals[null_mask] = poison
    return Col(kind, vals, ~null_mask)


def concat_cols(pages):
    """concatenate a list of pages (lists of Col) column by column"""
    out = []
    for c in range(len(pages[0])):
        parts = [p[c] for p in pages]
        kind = parts[0].kind
        if kind == "str":
            vals = [v for p in parts for v in p.values]
        else:
            vals = np.concatenate([p.values for p in parts])
        if all(p.valid is None for p in parts):
            valid = None
        else:
            valid = np.concatenate([np.ones(len(p), bool) if p.valid is None
                                    else p.valid for p in parts])
        out.append(Col(kind, vals, valid))
    return out


def split_pages(cols, sizes, bitmaps=None):
    """cut columns into pages of the given sizes; bitmaps[i] False strips the
    validity bitmaps of page i (its rows must then all be valid)"""
    assert sum(sizes) == len(cols[0])
    pages, at = [], 0
    for i, n in enumerate(sizes):
        keep = True if bitmaps is None else bitmaps[i]
        pages.append([c.slice(at, at + n, keep) for c in cols])
        at += n
    return pages


def keys_of(cols, channels):
    return [tuple(cols[c].cell(i) for c in channels) for i in range(len(cols[0]))]


def pack_bits(valid):
    n = len(valid)
    b = np.zeros(max((n + 63) // 64, 1) * 64, bool)
    b[:n] = valid
    return np.packbits(b, bitorder="little").view(np.uint64).copy()


def unpack_bits(words, n):
    if words is None:
        return np.ones(n, bool)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def tg_types(ops, cols):
    m = {"i64": ops.TG_BIGINT, "i32": ops.TG_INTEGER, "i16": ops.TG_SMALLINT,
         "i8": ops.TG_TINYINT, "f64": ops.TG_DOUBLE, "date": ops.TG_DATE,
         "str": ops.TG_VARCHAR}
    return [m[c.kind] for c in cols]


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
        if c.kind == "date":
            page.blocks[i].type = ops.TG_DATE
    return page


def output_cols(ops, pages, n_cols, gathered=True):
    """downloaded output pages -> list of Col (valid always a bool array),
    checking the VARCHAR offsets of every page on the way; in a gathered
    column a NULL VARCHAR cell has zero length (a semi join passes its probe
    columns through as they came)"""
    kinds = {ops.TG_BIGINT: "i64", ops.TG_INTEGER: "i32", ops.TG_SMALLINT: "i16",
             ops.TG_TINYINT: "i8", ops.TG_DOUBLE: "f64", ops.TG_DATE: "date",
             ops.TG_BOOLEAN: "i8", ops.TG_VARCHAR: "str"}
    out = []
    for c in range(n_cols):
        kind = kinds[pages[0][c]["type"]]
        vals, valid = [], []
        for p in pages:
            col = p[c]
            n = len(col["values"])
            v = unpack_bits(col["valid"], n)
            if kind == "str":
                offs = col["offsets"].astype(np.int64)
                lens = np.array([len(x) for x in col["values"]], np.int64)
                assert offs[0] == 0
                assert np.array_equal(np.diff(offs), lens)
                assert len(col["bytes"]) == offs[n]
                if gathered:
                    assert not lens[~v].any(), "a NULL VARCHAR cell has bytes"
                vals.extend(col["values"])
            else:
                vals.append(col["values"])
            valid.append(v)
        if kind != "str":
            vals = np.concatenate(vals) if vals else np.empty(0, _NP[kind])
        out.append(Col(kind, vals, np.concatenate(valid) if valid else None))
    return out


def assert_col_equal(got, src, idx, what):
    """got == src gathered by idx (-1 = NULL row), bit for bit: validity
    everywhere, values wherever valid"""
    idx = np.asarray(idx, np.int64)
    hit = idx >= 0
    safe = np.where(hit, idx, 0)
    src_valid = np.ones(len(src), bool) if src.valid is None else src.valid
    exp_valid = hit & (src_valid[safe] if len(src) else False)
    assert np.array_equal(got.valid, exp_valid), f"{what}: validity"
    assert got.kind == src.kind, what
    if src.kind == "str":
        exp = [src.values[i] for i in safe] if len(src) else [b""] * len(idx)
        bad = [k for k in np.flatnonzero(exp_valid) if got.values[k] != exp[k]]
    else:
        view = np.int64 if src.kind == "f64" else _NP[src.kind]
        exp = src.values[safe] if len(src) else np.zeros(len(idx), _NP[src.kind])
        bad = np.flatnonzero((got.values.view(view) != exp.view(view)) & exp_valid)
    assert len(bad) == 0, f"{what}: values differ first at output row {bad[0]}"


# --------------------------------------------------------------------------
# runner
# --------------------------------------------------------------------------
def build_bridge(sess, ops, build_pages, bkeys, bout, set_builder=False,
                 request_bitmap=False):
    bridge = ops.JoinBridge(sess)
    try:
        types = tg_types(ops, build_pages[0])
        if set_builder:
            build = ops.set_builder(sess, bridge, types, bkeys[0])
        else:
            build = ops.hash_builder(sess, bridge, types, bkeys, bout)
        try:
            if request_bitmap:
                ops.request_bitmap(bridge)
            for p in build_pages:
                build.add_input(make_page(ops, p))
            build.drain()
        finally:
            build.close()
    except Exception:
        bridge.close()
        raise
    return bridge


def probe_join(sess, ops, bridge, build_cols, bkeys, bout, probe_pages, pkeys,
               pout, outer, order=ORDER, pairs=None):
    """probe with all pages through ONE operator and check the concatenated
    output against the reference. The last probe and build output columns
    must be the BIGINT row numbers."""
    probe_cols = concat_cols(probe_pages)
    op = ops.lookup_join(sess, bridge, tg_types(ops, probe_pages[0]), pkeys,
                         pout, join_type=1 if outer else 0)
    try:
        for p in probe_pages:
            op.add_input(make_page(ops, p))
        pages = op.drain()
    finally:
        op.close()
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


def join_case(sess, ops, build_pages, bkeys, bout, probe_pages, pkeys, pout,
              outer, **kw):
    bridge = build_bridge(sess, ops, build_pages, bkeys, bout,
                          request_bitmap=kw.pop("request_bitmap", False))
    try:
        return probe_join(sess, ops, bridge, concat_cols(build_pages), bkeys,
                          bout, probe_pages, pkeys, pout, outer, **kw)
    finally:
        bridge.close()


def probe_semi(sess, ops, bridge, build_cols, bkey, probe_pages, pkey, expect=None):
    probe_cols = concat_cols(probe_pages)
    op = ops.semi_join(sess, bridge, pkey)
    try:
        for p in probe_pages:
            op.add_input(make_page(ops, p))
        pages = op.drain()
    finally:
        op.close()
    assert len(pages) == len(probe_pages)
    ncol = len(probe_cols)
    got = output_cols(ops, pages, ncol + 1, gathered=False)
    m = len(probe_cols[0])
    ident = np.arange(m, dtype=np.int64)
    for c in range(ncol):                         # probe channels pass through
        assert_col_equal(got[c], probe_cols[c], ident, f"probe channel {c}")
    if expect is None:
        ref = ref_semi(keys_of(build_cols, [bkey]), keys_of(probe_cols, [pkey]))
        hit = np.array([r is True for r in ref], bool)
        null = np.array([r is None for r in ref], bool)
    else:
        hit, null = expect
    match = got[ncol]
    assert len(match) == m
    assert np.array_equal(match.valid, ~null), "semi join: match validity"
    assert np.array_equal(match.values[~null], hit[~null].astype(np.int8)), \
        "semi join: match value"


def semi_case(sess, ops, build_pages, bkey, probe_pages, pkey, source="hash",
              **kw):
    bridge = build_bridge(sess, ops, build_pages, [bkey], [],
                          set_builder=(source == "set"),
                          request_bitmap=kw.pop("request_bitmap", False))
    try:
        probe_semi(sess, ops, bridge, concat_cols(build_pages), bkey,
                   probe_pages, pkey, **kw)
    finally:
        bridge.close()


# --------------------------------------------------------------------------
# single BIGINT key shapes: (bk, bnull, pk, pnull); null masks may be None
# --------------------------------------------------------------------------
_K = np.int64(-7046029254386353131)      # odd: g -> g * _K is injective mod 2^64


def key_of(g):
    """injective index -> BIGINT key, signed and spread over the int64 range"""
    return (np.asarray(g, np.int64) + np.int64(1)) * _K


def _probe_half(r, present, m, miss_base):
    """m probe keys, even rows drawn from `present` (hits), odd rows from
    indexes no build row uses (misses); empty `present` gives all misses"""
    pk = key_of(miss_base + np.arange(m))
    if len(present):
        pk[0::2] = r.choice(present, len(pk[0::2]))
    return pk


def shape_unique(nb, m, seed=0):
    """unique build keys, sparse, signed and mostly outside +-2^31; half the
    probe rows hit, half miss"""
    r = rng(seed)
    bk = key_of(r.permutation(nb))
    return bk, None, _probe_half(r, bk, m, 10 * nb + 7), None


def shape_dups(nb, m, seed=0):
    """1 to 4 copies of each key, shuffled; half the probe rows hit"""
    r = rng(seed)
    g = np.repeat(np.arange(nb), (np.arange(nb) % 4) + 1)[:nb]
    bk = key_of(r.permutation(g))
    return bk, None, _probe_half(r, bk, m, 10 * nb + 7), None


ONE_HOT_COPIES = 500


def shape_one_hot(nb, m, seed=0):
    """one key on 500 build rows among unique others: a long bucket for
    k_jc_sort and a long descending walk; a quarter of the probe asks for it"""
    assert nb >= ONE_HOT_COPIES
    r = rng(seed)
    g = np.arange(nb)
    g[:ONE_HOT_COPIES] = 0
    bk = key_of(r.permutation(g))
    pk = _probe_half(r, bk, m, 10 * nb + 7)
    pk[0::4] = key_of(0)
    return bk, None, pk, None


def colliding_keys(capacity, exclude_slot_of=()):
    """five distinct keys sharing one slot at `capacity` (A, B, C present, D
    and D2 spare), found by searching the integers"""
    cand = np.arange(1, 16 * capacity + 1, dtype=np.int64)
    s = slots_of(cand, capacity)
    counts = np.bincount(s, minlength=capacity)
    slot = int(np.argmax(counts >= 5))
    assert counts[slot] >= 5
    return cand[s == slot][:5], slot


def shape_colliding(nb, m, seed=0):
    """keys A (3 copies), B (1 copy) and C (2 copies) share one slot at the
    build's capacity; the probe asks for A, B, C, for D which lands in that
    slot but is absent, and for E which lands in an empty slot. Pins the
    three head encodings of k_probe_count (-2-row, -1 in a non-empty bucket,
    the slot itself) and the filtered descending walk of k_probe_fill."""
    assert nb >= 6
    r = rng(seed)
    cap = join_hash_size(nb)
    (a, b, c, d, _), slot = colliding_keys(cap)
    fill = np.arange(5 * 10 ** 7, 5 * 10 ** 7 + 64 * nb, dtype=np.int64)
    fill = fill[slots_of(fill, cap) != slot][:nb - 6]
    bk = r.permutation(np.concatenate([[a, a, a, b, c, c], fill]).astype(np.int64))
    e_cand = np.arange(10 ** 8, 10 ** 8 + 64 * cap, dtype=np.int64)
    used = np.zeros(cap, bool)
    used[slots_of(bk, cap)] = True
    e = e_cand[~used[slots_of(e_cand, cap)]][0]
    pk = np.resize(np.array([a, d, b, e, c, a, fill[0] if len(fill) else d, d],
                            np.int64), m)
    return bk, None, pk, None


def shape_all_miss(nb, m, seed=0):
    """no probe key is in the build: 0 rows inner, m rows outer"""
    r = rng(seed)
    return key_of(r.permutation(nb)), None, key_of(10 * nb + 7 + np.arange(m)), None


def shape_all_null_probe(nb, m, seed=0):
    """every probe key is NULL over a key the build holds: 0 rows inner, m
    rows outer"""
    r = rng(seed)
    bk = key_of(r.permutation(nb))
    pk = r.choice(bk, m) if nb else key_of(np.arange(m))
    return bk, None, pk, np.ones(m, bool)


def shape_nulls(nb, m, seed=0):
    """dups with about 3 % NULL keys on both sides (at least one each when
    the side has rows); a NULL build row keeps a key that the probe asks
    for, a NULL probe row a key that the build holds"""
    r = rng(seed)
    bk, _, pk, _ = shape_dups(nb, m, seed)
    bnull, pnull = r.random(nb) < 0.03, r.random(m) < 0.03
    if nb:
        bnull[nb // 2] = True
        pk[-1] = bk[nb // 2]             # asks for the key under the NULL
    if m and nb:
        pnull[m // 2] = True
        pk[m // 2] = bk[0]
    return bk, bnull, pk, pnull


SHAPES = {"unique": shape_unique, "dups": shape_dups, "one_hot": shape_one_hot,
          "colliding": shape_colliding, "all_miss": shape_all_miss,
          "all_null_probe": shape_all_null_probe, "nulls": shape_nulls}
MIN_BUILD = {"one_hot": ONE_HOT_COPIES, "colliding": 6}
CORE_SHAPES = ("unique", "dups", "colliding", "nulls")


def bigint_tables(bk, bnull, pk, pnull, payload_nulls=True):
    """build [key, payload, row] and probe [key, row] columns for one
    single-key shape; payload has its own NULLs over POISON_I"""
    nb, m = len(bk), len(pk)
    brow, prow = np.arange(nb, dtype=np.int64), np.arange(m, dtype=np.int64)
    key = Col("i64", bk) if bnull is None else Col("i64", bk, ~bnull)
    pay = brow * 7 + 3
    pay_c = nullable("i64", pay, brow % 11 == 5, POISON_I) if payload_nulls \
        else Col("i64", pay)
    pkey = Col("i64", pk) if pnull is None else Col("i64", pk, ~pnull)
    return [key, pay_c, Col("i64", brow)], [pkey, Col("i64", prow)]


def single_key_case(sess, ops, shape, nb, m, outer, build_sizes=None,
                    probe_sizes=None, **kw):
    build, probe = bigint_tables(*SHAPES[shape](nb, m, seed=nb + m))
    bpages = split_pages(build, build_sizes or [nb])
    ppages = split_pages(probe, probe_sizes or [m])
    return join_case(sess, ops, bpages, [0], [0, 1, 2], ppages, [0], [0, 1],
                     outer, **kw)


SMALL_CASES = [(s, nb) for s in SHAPES for nb in SMALL_BUILDS
               if nb >= MIN_BUILD.get(s, 0)]
EDGE_CASES = [(s, nb) for s in ("unique", "dups")
              for nb in REGION_BUILDS + LOAD_BUILDS]
CORE_CASES = [(s, nb) for s in CORE_SHAPES for nb in (65, 1000, 8193)]


# --------------------------------------------------------------------------
# core subset: also run under TG_JOIN_KV=1 and TG_JOIN_CSR=0 in child
# processes (both variables are read once per process)
# --------------------------------------------------------------------------
@pytest.mark.parametrize("outer", [False, True], ids=["inner", "outer"])
@pytest.mark.parametrize("shape,nb", CORE_CASES)
def test_core_lookup(sess, ops, shape, nb, outer):
    single_key_case(sess, ops, shape, nb, SMALL_M, outer)


@pytest.mark.parametrize("shape,nb", CORE_CASES)
def test_core_semi(sess, ops, shape, nb):
    build, probe = bigint_tables(*SHAPES[shape](nb, SMALL_M, seed=nb))
    semi_case(sess, ops, [build], 0, [probe], 0)


def test_core_generic_keys_need_csr(sess, ops):
    """a generic-key build works on the CSR table and is rejected with
    TG_ERR_UNSUPPORTED on the legacy one (TG_JOIN_CSR=0)"""
    import trino_amd
    build = [Col("i32", [3, 4, 3]), Col("i64", [0, 1, 2])]
    probe = [Col("i32", [3, 5]), Col("i64", [0, 1])]
    if CSR:
        join_case(sess, ops, [build], [0], [0, 1], [probe], [0], [0, 1], False)
    else:
        with pytest.raises(trino_amd.TrinoGpuError) as ei:
            build_bridge(sess, ops, [build], [0], [0, 1])
        assert str(ei.value).startswith(f"status {TG_ERR_UNSUPPORTED}:")
        assert "CSR" in str(ei.value)


def _run_child(env):
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x",
           "-k", "test_core", "-p", "no:cacheprovider"]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, **env), cwd=_ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
    except subprocess.TimeoutExpired:
        pytest.exit(f"join matrix child {env} hit its time limit: nothing "
                    "more is started on the GPU", returncode=3)
    if r.returncode < 0 or r.returncode >= 128:
        pytest.exit(f"join matrix child {env} ended on a signal "
                    f"(status {r.returncode}): nothing more is started on the "
                    f"GPU\n{r.stdout[-3000:]}", returncode=3)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:]


def test_variant_kv_table():
    """core subset under TG_JOIN_KV=1 (k_build_slotkv, the t.kv branches of
    k_probe_count and k_semi_probe): full list-order contract"""
    _run_child({"TG_JOIN_KV": "1"})


def test_variant_legacy_table():
    """core subset under TG_JOIN_CSR=0 (k_join_init, k_join_build, the legacy
    branches of the probe kernels): pairs of each probe row as a set"""
    _run_child({"TG_JOIN_CSR": "0"})


# --------------------------------------------------------------------------
# single BIGINT key
# --------------------------------------------------------------------------
@pytest.mark.parametrize("outer", [False, True], ids=["inner", "outer"])
@pytest.mark.parametrize("shape,nb", SMALL_CASES)
def test_single_key_small(sess, ops, shape, nb, outer):
    got = single_key_case(sess, ops, shape, nb, SMALL_M, outer)
    if shape in ("all_miss", "all_null_probe"):
        assert len(got[0]) == (SMALL_M if outer else 0)


@pytest.mark.parametrize("outer", [False, True], ids=["inner", "outer"])
@pytest.mark.parametrize("shape,nb", EDGE_CASES)
def test_region_and_load_factor_edges(sess, ops, shape, nb, outer):
    """8192 | 8193 rows: one | two regions of JREG_SLOTS; 65536 | 65537 rows:
    the load-factor step of join_hash_size"""
    single_key_case(sess, ops, shape, nb, 1000, outer)


@pytest.mark.parametrize("outer", [False, True], ids=["inner", "outer"])
def test_one_hot_two_regions(sess, ops, outer):
    single_key_case(sess, ops, "one_hot", 8193, SMALL_M, outer)


@pytest.mark.parametrize("outer", [False, True], ids=["inner", "outer"])
@pytest.mark.parametrize("m", PROBE_EDGES)
def test_probe_page_edges(sess, ops, m, outer):
    """probe pages around JSCAN_CHUNK against an 8193-row dups build: the
    two-level scan across one, two and three chunks"""
    single_key_case(sess, ops, "dups", 8193, m, outer)


@pytest.mark.parametrize("outer", [False, True], ids=["inner", "outer"])
def test_several_probe_pages_in_order(sess, ops, outer):
    single_key_case(sess, ops, "nulls", 1000, 65 + 0 + 1 + 700 + 64, outer,
                    probe_sizes=[65, 0, 1, 700, 64])


# ---- the 2^20-row build: inputs and reference shared, computed once ----
@functools.lru_cache(None)
def big_inputs():
    r = rng(20)
    nb, m = BIG_BUILD, GRID_STRIDE_M
    g = np.repeat(np.arange(nb), (np.arange(nb) % 4) + 1)[:nb]
    bk = key_of(r.permutation(g))
    bnull = r.random(nb) < 0.03
    pk = key_of(10 * nb + 7 + np.arange(m))
    pk[0::2] = r.choice(bk, len(pk[0::2]))
    pnull = r.random(m) < 0.03
    for a in (bk, bnull, pk, pnull):
        a.setflags(write=False)
    return bk, bnull, pk, pnull


@functools.lru_cache(None)
def big_reference():
    bk, bnull, pk, pnull = big_inputs()
    pairs = ref_join_vec(bk, ~bnull, pk, ~pnull)
    for a in pairs:
        a.setflags(write=False)
    return pairs


def big_case(sess, ops):
    build, probe = bigint_tables(*big_inputs(), payload_nulls=False)
    join_case(sess, ops, [build], [0], [0, 1, 2], [probe], [0], [0, 1], False,
              pairs=big_reference(), order="list")


def test_big_build_classic(sess, ops):
    """2^20 build rows: capacity 2^21, 64 regions, second load-factor step,
    a second stride in every build kernel and in the probe kernels"""
    big_case(sess, ops)


def test_big_build_partitioned(sess, ops, partitioned):
    """the same through the partitioned probe: a 20 MB table = 2 partitions"""
    c = source_constants()
    tbl_bytes = join_hash_size(BIG_BUILD) * 4 + BIG_BUILD * 12
    assert c["PART_BYTES"] < tbl_bytes <= 2 * c["PART_BYTES"]
    big_case(sess, ops)


def test_big_build_semi(sess, ops):
    bk, bnull, pk, pnull = big_inputs()
    build, probe = bigint_tables(bk, bnull, pk, pnull, payload_nulls=False)
    semi_case(sess, ops, [build], 0, [probe], 0,
              expect=ref_semi_vec(bk, ~bnull, pk, ~pnull))


# --------------------------------------------------------------------------
# partitioned probe against the reference (one partition at these sizes)
# --------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 65, SMALL_M])
@pytest.mark.parametrize("shape,nb", [(s, nb) for s in
                                      ("unique", "dups", "colliding", "nulls",
                                       "all_miss", "all_null_probe")
                                      for nb in (65, 1000)] + [("dups", 8193)])
def test_partitioned_probe(sess, ops, partitioned, shape, nb, m):
    single_key_case(sess, ops, shape, nb, m, False, order="list")


def overflow_inputs():
    """64 build rows and 64 probe rows of one key: 4096 matches against the
    first-try cap of probe rows + build rows + 64, so the exact retry runs"""
    k = key_of(np.full(OVERFLOW_N, 5))
    return k, None, k.copy(), None


def test_partitioned_probe_overflow_retry(sess, ops, partitioned):
    build, probe = bigint_tables(*overflow_inputs())
    got = join_case(sess, ops, [build], [0], [0, 1, 2], [probe], [0], [0, 1],
                    False, order="list")
    assert len(got[0]) == OVERFLOW_N * OVERFLOW_N > 3 * OVERFLOW_N


# --------------------------------------------------------------------------
# multi-page builds
# --------------------------------------------------------------------------
MULTI_PAGE_SIZES = [37, 64, 0, 1, 100, 8000]
MULTI_PAGE_BITMAPS = [False, True, False, False, True, True]


def _multi_page_null_rows():
    """global build rows that are NULL: only inside pages that carry a bitmap,
    first and last row of such pages included"""
    starts = np.cumsum([0] + MULTI_PAGE_SIZES)
    rows = []
    for i, (n, bm) in enumerate(zip(MULTI_PAGE_SIZES, MULTI_PAGE_BITMAPS)):
        if bm and n:
            lo = int(starts[i])
            rows += [lo, lo + n - 1] + list(range(lo + 3, lo + n, 29))
    return np.array(sorted(set(rows)))


def _multi_page_masks(shift):
    """(key NULL mask, output-column NULL mask): the second is the first
    moved by `shift` rows, cleared in the pages that carry no bitmap"""
    nb = sum(MULTI_PAGE_SIZES)
    knull = np.zeros(nb, bool)
    knull[_multi_page_null_rows()] = True
    vnull = np.roll(knull, shift)
    starts = np.cumsum([0] + MULTI_PAGE_SIZES)
    for i, bm in enumerate(MULTI_PAGE_BITMAPS):
        if not bm:
            vnull[starts[i]:starts[i + 1]] = False
    return knull, vnull


@pytest.mark.parametrize("outer", [False, True], ids=["inner", "outer"])
def test_multi_page_build_bigint(sess, ops, outer):
    """pages of 37, 64, 0, 1, 100 and 8000 rows, NULLs in the key and in a
    non-key output column, bitmaps on some pages only: k_bitmap_concat at odd
    bit offsets and the flat key copy"""
    nb = sum(MULTI_PAGE_SIZES)
    bk, _, pk, pnull = shape_nulls(nb, 1000, seed=3)
    knull, vnull = _multi_page_masks(1)
    brow = np.arange(nb, dtype=np.int64)
    pk[3] = bk[_multi_page_null_rows()[0]]
    build = [Col("i64", bk, ~knull), nullable("i32", brow % 1000 - 500, vnull, 2 ** 30 + 1),
             Col("i64", brow)]
    probe = [Col("i64", pk, ~pnull), Col("i64", np.arange(1000))]
    bpages = split_pages(build, MULTI_PAGE_SIZES, MULTI_PAGE_BITMAPS)
    join_case(sess, ops, bpages, [0], [0, 1, 2], [probe], [0], [0, 1], outer)


def _words(idx):
    """distinct short byte strings, prefixes of one another among them"""
    return [b"k" * (int(i) % 5) + str(int(i) // 5).encode() for i in idx]


def multi_page_varchar_case(sess, ops, outer):
    """the multi-page build with a VARCHAR key and a VARCHAR output column,
    checked against ref_join"""
    nb = sum(MULTI_PAGE_SIZES)
    r = rng(4)
    g = r.permutation(np.repeat(np.arange(nb), (np.arange(nb) % 3) + 1)[:nb])
    knull, vnull = _multi_page_masks(2)
    brow = np.arange(nb, dtype=np.int64)
    build = [nullable("str", _words(g), knull, POISON_S),
             nullable("str", [b"v%d" % (i % 97) * (i % 4) for i in range(nb)],
                      vnull, POISON_S),
             Col("i64", brow)]
    m = 1000
    pg = np.where(np.arange(m) % 2 == 0, r.choice(g, m), nb + np.arange(m))
    pg[5] = g[_multi_page_null_rows()[0]]
    probe = [nullable("str", _words(pg), np.arange(m) % 31 == 7, POISON_S),
             Col("i64", np.arange(m))]
    bpages = split_pages(build, MULTI_PAGE_SIZES, MULTI_PAGE_BITMAPS)
    return join_case(sess, ops, bpages, [0], [0, 1, 2], [probe], [0], [0, 1], outer)


@pytest.mark.parametrize("outer", [False, True], ids=["inner", "outer"])
def test_multi_page_build_varchar(sess, ops, outer):
    """the same with a VARCHAR key and a VARCHAR output column: concat_varchar
    and k_off_rebase"""
    multi_page_varchar_case(sess, ops, outer)


# --------------------------------------------------------------------------
# generic keys
# --------------------------------------------------------------------------
NAN_A = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), np.float64)[0]
NAN_B = np.frombuffer(np.uint64(0xFFF8000000000ABC).tobytes(), np.float64)[0]


def generic_tables(name):
    """(build cols, build key channels, probe cols, probe key channels);
    the last column of each side is the row number"""
    r = rng(11)
    if name == "bigint_integer":
        nb, m = 600, 500
        a = key_of(r.integers(0, 40, nb))
        b = r.integers(-3, 3, nb)
        build = [nullable("i64", a, np.arange(nb) % 17 == 3),
                 nullable("i32", b, np.arange(nb) % 19 == 4)]
        pa, pb = r.choice(a, m), r.integers(-3, 3, m)
        probe = [nullable("i64", pa, np.arange(m) % 23 == 5),
                 nullable("i32", pb, np.arange(m) % 13 == 6)]
    elif name == "varchar_bigint":
        words = [b"", b"a", b"ab", b"abc", b"abcd", b"abcdefgh", b"abcdefghi",
                 b"b", b"ab\0", b"abcdefghijklmnopqrstuvwxyz0123456789"]
        nb, m = 400, 300
        wi, n = r.integers(0, len(words), nb), r.integers(0, 3, nb)
        build = [nullable("str", [words[i] for i in wi], np.arange(nb) % 29 == 2,
                          b""),
                 Col("i64", n)]
        pwi, pn = r.integers(0, len(words), m), r.integers(0, 4, m)
        probe = [nullable("str", [words[i] for i in pwi], np.arange(m) % 31 == 1,
                          b"a"),
                 Col("i64", pn)]
    elif name == "smallint_tinyint_date":
        nb, m = 500, 400
        build = [Col("i16", r.integers(-3, 2, nb) * 10000),
                 Col("i8", r.integers(-2, 2, nb) * 60),
                 Col("date", r.integers(-2, 2, nb) * 100000)]
        probe = [Col("i16", r.integers(-3, 4, m) * 10000),
                 Col("i8", r.integers(-2, 3, m) * 60),
                 Col("date", r.integers(-2, 3, m) * 100000)]
    elif name == "double":
        vals = np.array([-0.0, 0.0, NAN_A, NAN_B, np.inf, -np.inf, 1.5, -1.5,
                         5e-324, 1e308])
        nb, m = 300, 200
        bi, pi = r.integers(0, len(vals), nb), r.integers(0, len(vals), m)
        build = [nullable("f64", vals[bi], np.arange(nb) % 15 == 1, 1.5)]
        probe = [nullable("f64", vals[pi], np.arange(m) % 14 == 2, 0.0)]
    elif name == "integer":
        nb, m = 1000, 700
        build = [nullable("i32", r.integers(-50, 50, nb) * 40000000,
                          np.arange(nb) % 37 == 3, 0)]
        probe = [nullable("i32", r.integers(-53, 54, m) * 40000000,
                          np.arange(m) % 41 == 3, 0)]
    else:
        raise KeyError(name)
    nkeys = len(build)
    build.append(Col("i64", np.arange(len(build[0]))))
    probe.append(Col("i64", np.arange(len(probe[0]))))
    return build, list(range(nkeys)), probe, list(range(nkeys))


GENERIC = ("bigint_integer", "varchar_bigint", "smallint_tinyint_date",
           "double", "integer")


@pytest.mark.parametrize("outer", [False, True], ids=["inner", "outer"])
@pytest.mark.parametrize("name", GENERIC)
def test_generic_keys(sess, ops, name, outer):
    build, bk, probe, pk = generic_tables(name)
    allc = list(range(len(build)))
    join_case(sess, ops, [build], bk, allc, [probe], pk,
              list(range(len(probe))), outer)


def test_nan_keys_do_not_match(sess, ops):
    """defect C: DOUBLE keys compare with IEEE ==. NaN of either bit pattern
    matches nothing, -0.0 matches 0.0"""
    build = [Col("f64", [NAN_A, 0.0, NAN_B, -0.0, 2.0]), Col("i64", np.arange(5))]
    probe = [Col("f64", [NAN_A, NAN_B, -0.0, 0.0, 2.0]), Col("i64", np.arange(5))]
    got = join_case(sess, ops, [build], [0], [0, 1], [probe], [0], [0, 1], False)
    assert list(zip(got[1].values.tolist(), got[3].values.tolist())) == \
        [(2, 3), (2, 1), (3, 3), (3, 1), (4, 4)]
    semi_case(sess, ops, [build], 0, [probe], 0)


# --------------------------------------------------------------------------
# outer-join output columns
# --------------------------------------------------------------------------
def outer_column_tables(source_nulls):
    nb, m = 300, 257
    bk, _, pk, _ = shape_dups(nb, m, seed=8)
    i = np.arange(nb)
    specs = [("i64", i * 1000003 - 5, POISON_I), ("f64", i * 0.5 - 7, 1e300),
             ("i32", i * 7001 - 9, 2 ** 30 + 1), ("date", 9000 + i, 2 ** 30 + 2),
             ("i16", i * 11 - 1000, 31000), ("i8", i % 100 - 50, 111),
             ("str", [b"w%d" % k * (k % 3) for k in range(nb)], POISON_S)]
    cols = [Col("i64", bk)]
    for j, (kind, vals, poison) in enumerate(specs):
        if source_nulls:
            cols.append(nullable(kind, vals, i % (5 + j) == 1, poison))
        else:
            cols.append(Col(kind, vals))
    cols.append(Col("i64", i))
    return cols, [Col("i64", pk), Col("i64", np.arange(m))]


@pytest.mark.parametrize("source_nulls", [False, True], ids=["dense", "nulls"])
def test_outer_join_build_columns_every_width(sess, ops, source_nulls):
    """build output columns of 8, 4, 2 and 1 bytes and VARCHAR (k_gather and
    run_gather_var with null positions): the NULL build side of an unmatched
    probe row has a cleared validity bit in every one of them"""
    build, probe = outer_column_tables(source_nulls)
    allc = list(range(len(build)))
    got = join_case(sess, ops, [build], [0], allc, [probe], [0], [0, 1], True)
    miss = ~got[-1].valid
    assert miss.any() and not miss.all()
    for c in got[2:]:
        assert not c.valid[miss].any()


def test_outer_join_varchar_build_column_is_null(sess, ops):
    """defect B: an unmatched probe row gets NULL, not '', in a VARCHAR build
    column that has no NULLs of its own"""
    build = [Col("i64", [1, 2, 2]), Col("str", [b"one", b"two", b"deux"]),
             Col("i64", np.arange(3))]
    probe = [Col("i64", [2, 7, 1]), Col("i64", np.arange(3))]
    got = join_case(sess, ops, [build], [0], [1, 2], [probe], [0], [0, 1], True)
    assert got[2].values == [b"deux", b"two", b"", b"one"]
    assert got[2].valid.tolist() == [True, True, False, True]


# --------------------------------------------------------------------------
# empty build
# --------------------------------------------------------------------------
def _empty(cols):
    return [c.slice(0, 0, False) for c in cols]


@pytest.mark.parametrize("pages", ["no_page", "empty_page"])
@pytest.mark.parametrize("name", ["bigint"] + list(GENERIC))
def test_empty_build(sess, ops, name, pages):
    """defect A for the generic keys: inner gives 0 rows, outer m rows that
    are all build-side NULL, semi all False and valid, NULL probes included"""
    if name == "bigint":
        build, probe = bigint_tables(*shape_nulls(8, SMALL_M, seed=1))
        bk = pk = [0]
    else:
        build, bk, probe, pk = generic_tables(name)
    bpages = [_empty(build)]
    allb, allp = list(range(len(build))), list(range(len(probe)))
    for outer in (False, True):
        bridge = ops.JoinBridge(sess)
        try:
            b = ops.hash_builder(sess, bridge, tg_types(ops, build), bk, allb)
            if pages == "empty_page":
                b.add_input(make_page(ops, bpages[0]))
            b.drain()
            b.close()
            got = probe_join(sess, ops, bridge, bpages[0], bk, allb, [probe],
                             pk, allp, outer)
            assert len(got[0]) == (len(probe[0]) if outer else 0)
            for c in got[len(allp):]:
                assert not c.valid.any()
            if len(bk) == 1:
                probe_semi(sess, ops, bridge, bpages[0], bk[0], [probe], pk[0])
        finally:
            bridge.close()


# --------------------------------------------------------------------------
# semi join
# --------------------------------------------------------------------------
def semi_tables(key, shape, build_null, nb=1000, m=SMALL_M):
    bk, _, pk, _ = SHAPES[shape](nb, m, seed=5)
    bnull = np.zeros(nb, bool)
    if build_null:
        bnull[[1, nb // 2]] = True
    pnull = np.arange(m) % 37 == 9
    if key == "bigint":
        conv = lambda a: ("i64", a, POISON_I)
    elif key == "double":
        # distinct int64 keys stay distinct: small indexes scaled by 0.25
        lut = {int(k): i for i, k in enumerate(np.unique(np.concatenate([bk, pk])))}
        conv = lambda a: ("f64", np.array([lut[int(k)] for k in a]) * 0.25 - 3, 0.0)
    else:
        conv = lambda a: ("str", [b"%x" % (int(k) & (2 ** 64 - 1)) for k in a], b"")
    kind, bv, _ = conv(bk)
    _, pv, _ = conv(pk)
    # under a NULL cell: the value itself, which would match if it were read
    build = [Col(kind, bv, ~bnull) if build_null else Col(kind, bv),
             Col("i64", np.arange(nb))]
    probe = [Col(kind, pv, ~pnull), Col("i64", np.arange(m))]
    return build, probe


@pytest.mark.parametrize("build_null", [False, True], ids=["dense", "null_key"])
@pytest.mark.parametrize("shape", ["colliding", "dups"])
@pytest.mark.parametrize("source,key", [("hash", "bigint"), ("hash", "double"),
                                        ("hash", "varchar"), ("set", "bigint")])
def test_semi_join(sess, ops, source, key, shape, build_null):
    """three-valued IN through hash_builder with a BIGINT key (CSR with
    csr_keys), with a DOUBLE and a VARCHAR key (generic CSR) and through
    set_builder (bitmap or, for these sparse keys, its index fallback)"""
    build, probe = semi_tables(key, shape, build_null)
    semi_case(sess, ops, [build], 0, [probe], 0, source=source)


def test_semi_join_grid_stride(sess, ops):
    bk, bnull, pk, pnull = shape_nulls(8193, GRID_STRIDE_M, seed=6)
    build, probe = bigint_tables(bk, bnull, pk, pnull)
    semi_case(sess, ops, [build], 0, [probe], 0,
              expect=ref_semi_vec(bk, ~bnull, pk, ~pnull))


# --------------------------------------------------------------------------
# set builder and k_set_bits
# --------------------------------------------------------------------------
def set_shapes():
    """name -> (build keys, null mask or None, expects_bitmap)"""
    r = rng(7)
    runs = np.sort(np.concatenate([np.repeat(np.arange(-700, -700 + 200), 9),
                                   np.arange(-300, 1000, 3)]))
    out = {
        # sorted, clustered: many lanes of one wave share a bitmap word
        "clustered": (np.sort(r.integers(-500, 1500, 3001)), None),
        # runs of equal and adjacent keys that cross word boundaries, key_min < 0
        "runs_cross_words": (runs, None),
        "range64": (np.concatenate([[100, 163], r.integers(100, 164, 131)]), None),
        "range65": (np.concatenate([[100, 164], r.integers(100, 165, 131)]), None),
        "range128": (np.concatenate([[-64, 63], r.integers(-64, 64, 131)]), None),
        "n_not_multiple_of_64": (np.sort(r.integers(0, 300, 197)), None),
        "nulls_inside_run": (np.repeat(np.arange(50, 90), 5),
                             np.arange(200) % 7 == 3),
        "one_row": (np.array([-5]), None),
    }
    return {k: (np.asarray(v[0], np.int64), v[1]) for k, v in out.items()}


SET_SHAPES = ("clustered", "runs_cross_words", "range64", "range65", "range128",
              "n_not_multiple_of_64", "nulls_inside_run", "one_row")
WIDE_RANGE_KEYS = (-2 ** 40, 0, 2 ** 40)


def check_key_range(ops, bridge, bk, bnull):
    valid = np.ones(len(bk), bool) if bnull is None else ~bnull
    mn, mx, cnt = ops.join_key_range(bridge)
    assert cnt == int(valid.sum())
    if cnt:
        assert (mn, mx) == (int(bk[valid].min()), int(bk[valid].max()))


@pytest.mark.parametrize("name", SET_SHAPES)
def test_set_builder_bitmap(sess, ops, name):
    bk, bnull = set_shapes()[name]
    lo, hi = int(bk.min()), int(bk.max())
    pk = np.arange(lo - 70, hi + 71, dtype=np.int64)       # every key and both edges
    build = [Col("i64", bk) if bnull is None else nullable("i64", bk, bnull, lo - 3)]
    probe = [nullable("i64", pk, np.arange(len(pk)) % 13 == 6, lo)]
    bridge = build_bridge(sess, ops, [build], [0], [], set_builder=True)
    try:
        check_key_range(ops, bridge, build[0].values, bnull)
        probe_semi(sess, ops, bridge, build, 0, [probe], 0)
    finally:
        bridge.close()


@pytest.mark.parametrize("build_null", [False, True], ids=["dense", "null_key"])
def test_set_builder_wide_range_falls_back_to_index(sess, ops, build_null):
    """key range > 2^33: no bitmap, the index answers and still agrees"""
    bk = np.concatenate([np.array(WIDE_RANGE_KEYS, np.int64), key_of(np.arange(200))])
    bnull = np.arange(len(bk)) == 5 if build_null else None
    pk = np.concatenate([bk, bk + 1, np.array([2 ** 40 - 1, -2 ** 40 - 1, 1])])
    build = [Col("i64", bk) if bnull is None else Col("i64", bk, ~bnull)]
    probe = [nullable("i64", pk, np.arange(len(pk)) % 13 == 6, 0)]
    bridge = build_bridge(sess, ops, [build], [0], [], set_builder=True)
    try:
        check_key_range(ops, bridge, bk, bnull)
        probe_semi(sess, ops, bridge, build, 0, [probe], 0)
    finally:
        bridge.close()


@pytest.mark.parametrize("source", ["set", "hash"])
def test_key_range_all_null_build(sess, ops, source):
    bk = np.arange(70, dtype=np.int64)
    build = [Col("i64", bk, np.zeros(70, bool))]
    probe = [nullable("i64", np.arange(-3, 80), np.arange(83) % 9 == 1, 5)]
    bridge = build_bridge(sess, ops, [build], [0], [], set_builder=(source == "set"))
    try:
        assert ops.join_key_range(bridge)[2] == 0
        probe_semi(sess, ops, bridge, build, 0, [probe], 0)
    finally:
        bridge.close()


@pytest.mark.parametrize("shape,nb", [("dups", 1000), ("nulls", 1000),
                                      ("colliding", 65), ("unique", 8193)])
def test_key_range_hash_builder(sess, ops, shape, nb):
    bk, bnull, pk, pnull = SHAPES[shape](nb, SMALL_M, seed=2)
    build, _ = bigint_tables(bk, bnull, pk, pnull)
    bridge = build_bridge(sess, ops, [build], [0], [0, 1, 2])
    try:
        check_key_range(ops, bridge, bk, bnull)
    finally:
        bridge.close()


# --------------------------------------------------------------------------
# dynamic-filter bitmap beside the index
# --------------------------------------------------------------------------
@pytest.mark.parametrize("build_null", [False, True], ids=["dense", "null_key"])
def test_requested_bitmap_beside_index(sess, ops, build_null):
    """request_bitmap before the build finishes: the lookup join on that
    bridge still equals ref_join, and the semi join, which then takes the
    bitmap branch with has_null_key from the CSR build, equals ref_semi"""
    r = rng(12)
    nb, m = 1000, 600
    bk = r.integers(-300, 900, nb).astype(np.int64)
    bnull = (np.arange(nb) % 50 == 7) if build_null else None
    pk = r.integers(-400, 1000, m).astype(np.int64)
    if build_null:
        only_null = 5000                # a key held by NULL build rows only
        bk[bnull] = only_null
        pk[:3] = only_null
    build, probe = bigint_tables(bk, bnull, pk, np.arange(m) % 17 == 2)
    bridge = build_bridge(sess, ops, [build], [0], [0, 1, 2], request_bitmap=True)
    try:
        check_key_range(ops, bridge, bk, bnull)
        for outer in (False, True):
            probe_join(sess, ops, bridge, build, [0], [0, 1, 2], [probe], [0],
                       [0, 1], outer)
        probe_semi(sess, ops, bridge, build, 0, [probe], 0)
    finally:
        bridge.close()


# --------------------------------------------------------------------------
# rejections (defects D and E): checked on the host before any kernel runs
# --------------------------------------------------------------------------
def _rejected(ops, op, page_cols, status, *words):
    import trino_amd
    try:
        with pytest.raises(trino_amd.TrinoGpuError) as ei:
            op.add_input(make_page(ops, page_cols))
    finally:
        op.close()
    msg = str(ei.value)
    assert msg.startswith(f"status {status}:"), msg
    for w in words:
        assert w in msg, msg


@pytest.fixture
def two_key_bridge(sess, ops):
    build = [Col("i64", [1, 2, 3]), Col("i32", [4, 5, 6]), Col("i64", [0, 1, 2])]
    bridge = build_bridge(sess, ops, [build], [0, 1], [2])
    yield bridge
    bridge.close()


def test_semi_join_rejects_multi_key_build(sess, ops, two_key_bridge):
    """defect D: the semi join carries one key channel"""
    _rejected(ops, ops.semi_join(sess, two_key_bridge, 0), [Col("i64", [1, 2])],
              TG_ERR_UNSUPPORTED, "single key channel", "2")


def test_lookup_join_rejects_key_count_mismatch(sess, ops, two_key_bridge):
    """defect E: fewer or more probe key channels than the build has"""
    T = ops.TG_BIGINT
    page = [Col("i64", [1, 2]), Col("i32", [4, 5]), Col("i32", [4, 5])]
    _rejected(ops, ops.lookup_join(sess, two_key_bridge, [T], [0], [0]), page,
              TG_ERR_INVALID_ARG, "1 join key channels", "build has 2")
    _rejected(ops, ops.lookup_join(sess, two_key_bridge, [T], [0, 1, 2], [0]), page,
              TG_ERR_INVALID_ARG, "3 join key channels", "build has 2")


def test_lookup_join_rejects_key_type_mismatch(sess, ops, two_key_bridge):
    """defect E: same count, another type in one position; VARCHAR against
    INTEGER would read through null offsets"""
    T = ops.TG_BIGINT
    _rejected(ops, ops.lookup_join(sess, two_key_bridge, [T, T], [0, 1], [0]),
              [Col("i64", [1, 2]), Col("i64", [4, 5])],
              TG_ERR_INVALID_ARG, "type mismatch", "key 1")
    _rejected(ops, ops.lookup_join(sess, two_key_bridge, [T, T], [0, 1], [0]),
              [Col("i64", [1, 2]), Col("str", [b"4", b"5"])],
              TG_ERR_INVALID_ARG, "type mismatch", "key 1")
    _rejected(ops, ops.lookup_join(sess, two_key_bridge, [T, T], [0, 5], [0]),
              [Col("i64", [1, 2]), Col("i32", [4, 5])],
              TG_ERR_INVALID_ARG, "outside the page")
    build = [Col("str", [b"a", b"b"]), Col("i64", [0, 1])]
    bridge = build_bridge(sess, ops, [build], [0], [1])
    try:
        _rejected(ops, ops.lookup_join(sess, bridge, [T], [0], [0]),
                  [Col("i32", [1, 2])], TG_ERR_INVALID_ARG, "type mismatch")
    finally:
        bridge.close()


@pytest.mark.parametrize("source", ["set", "hash"])
def test_semi_join_rejects_key_type_mismatch(sess, ops, source):
    """defect E in the semi join"""
    build = [Col("i64", [1, 2, 3])]
    bridge = build_bridge(sess, ops, [build], [0], [], set_builder=(source == "set"))
    try:
        _rejected(ops, ops.semi_join(sess, bridge, 0), [Col("i32", [1, 2])],
                  TG_ERR_INVALID_ARG, "type mismatch")
        _rejected(ops, ops.semi_join(sess, bridge, 0), [Col("str", [b"1", b"2"])],
                  TG_ERR_INVALID_ARG, "type mismatch")
    finally:
        bridge.close()
