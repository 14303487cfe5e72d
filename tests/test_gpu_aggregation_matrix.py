"""Aggregation parity matrix: hash, streaming and dense-range aggregation
against an exact reference written here (no oracle, no trino_amd
aggregation), with key shapes that steer every update path of k_agg_update /
k_agg_update_sorted, page sizes that reach the grid-stride loop, signed and
NULL inputs, masked aggregates and state growth with live MIN/MAX state.

Reference: rows are grouped by their Python key in first-occurrence order;
integer kinds use Python int arithmetic, SUM_F64_EXACT / SUM_F64 / AVG_F64 use
math.fsum (the correctly rounded exact sum). SQL NULL rules: NULL values are
skipped, a mask `a > b` with a NULL operand is not true, MIN/MAX/AVG (and, in
SQL, SUM) over no qualifying row are NULL (None here).

Comparison: integer kinds and the exact sum bit-equal; validity bitmaps
compared wherever the reference says NULL. SUM_F64 / AVG_F64 only: any
summation order has error <= (n_g-1)u S/(1-(n_g-1)u) with u = 2^-53,
S = sum|v_i|, n_g = rows in the group, so the tests assert
|got - fsum| <= n_g * 2^-53 * S (AVG: that over the count, plus
2^-53 * |avg| for the division). Bounds come from the reference's inputs only.

The operators emit 0 (no validity bitmap) for a SUM over no non-NULL input
where SQL says NULL: that recorded deviation is the single strict xfail
below; every other case builds inputs so each group has a non-NULL addend
and asserts it from the reference.

The host-side checks of the shape constructors and of this reference live in
tests/test_oracle_units.py (they need no GPU).
"""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

(COUNT_STAR, COUNT_COL, SUM_F64, SUM_I64, AVG_F64, SUM_F64_EXACT, MIN_I64,
 MAX_I64) = range(8)
SUM_KINDS = (SUM_F64, SUM_I64, SUM_F64_EXACT)
PARTIAL, FINAL, SINGLE = 0, 1, 2

WAVE = 64
GRID_THREADS = 2048 * 256            # tg_grid_for cap: blocks x block size
GRID_STRIDE_N = GRID_THREADS + 64 * 3 + 5   # 2nd stride iteration, partial last wave
SMALL_NS = (1, 63, 64, 65, 127, 1000)
U = 2.0 ** -53

POISON_I = 2 ** 62 + 12345           # data word under a NULL BIGINT cell
SP_WIDE, SP_MONEY = 20, 43


@pytest.fixture(scope="module")
def sess():
    import trino_amd
    s = trino_amd.Session(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ops():
    from trino_amd import ops
    assert (ops.AGG_COUNT_STAR, ops.AGG_COUNT_COL, ops.AGG_SUM_F64,
            ops.AGG_SUM_I64, ops.AGG_AVG_F64, ops.AGG_SUM_F64_EXACT,
            ops.AGG_MIN_I64, ops.AGG_MAX_I64) == tuple(range(8))
    assert (ops.STEP_PARTIAL, ops.STEP_FINAL, ops.STEP_SINGLE) == (0, 1, 2)
    return ops


def rng(seed=0):
    return np.random.default_rng(seed)


# --------------------------------------------------------------------------
# key shapes (group indexes per row; one wave = one aligned 64-row slice)
# --------------------------------------------------------------------------
POOL = 3     # slices cycle through POOL key sets, so waves share groups


def key_of(g):
    """injective group index -> BIGINT key (signed, not dense, not sorted)"""
    return (np.asarray(g, np.int64) - 3) * np.int64(2654435761) + np.int64(11)


def _lanes(n):
    i = np.arange(n, dtype=np.int64)
    return i // WAVE, i % WAVE


def shape_uniform(n):
    """every 64-row slice holds one key, changing at multiples of 64:
    wave-uniform path (one shuffle reduction, one atomic per wave)"""
    s, _ = _lanes(n)
    return 800 + s % 5


def shape_hot2(n):
    """2 keys per slice in contiguous clusters of 32 lanes: hot-group rounds,
    2 rounds, all lanes consumed by the rounds"""
    s, l = _lanes(n)
    return 500 + (s % POOL) * 2 + l // 32


def shape_hot8(n):
    """8 keys per slice in contiguous clusters of 8 lanes: hot-group rounds,
    exactly 8 rounds, first cluster == 8 (kept), nothing left over"""
    s, l = _lanes(n)
    return 600 + (s % POOL) * 8 + l // 8


def shape_hot_then_tail(n):
    """first cluster of 16 lanes then 48 distinct keys: round 1 kept, rounds
    2-8 take one lane each, the other 41 lanes are leftovers after rounds == 8"""
    s, l = _lanes(n)
    return np.where(l < 16, 300 + s % POOL, 400 + (s % POOL) * 48 + (l - 16))


def shape_bail(n):
    """first cluster of 7 lanes then mixed keys: exits on
    rounds == 1 && popc < 8, the other 57 lanes take per-lane atomics"""
    s, l = _lanes(n)
    return np.where(l < 7, 200 + s % POOL, 210 + (s % POOL) * 5 + l % 5)


def shape_interleaved(n):
    """two keys alternating lane by lane: hot-group rounds whose round-1
    cluster has 32 lanes that are not contiguous"""
    s, l = _lanes(n)
    return 700 + (s % POOL) * 2 + (l & 1)


def shape_scatter(n):
    """64 distinct keys per slice: first cluster of 1 lane, bail after round
    1, 63 per-lane atomics"""
    s, l = _lanes(n)
    return 1000 + (s % POOL) * 64 + l


def shape_single(n):
    """one key for the whole page (also the scalar aggregation case):
    wave-uniform path in every full wave"""
    return np.zeros(n, np.int64)


SHAPES = {
    "uniform": shape_uniform, "hot2": shape_hot2, "hot8": shape_hot8,
    "hot_then_tail": shape_hot_then_tail, "bail": shape_bail,
    "interleaved": shape_interleaved, "scatter": shape_scatter,
    "single": shape_single,
}

# what simulate_wave() must report for every FULL slice of the shape
SHAPE_PATHS = {
    "uniform": dict(path="uniform"),
    "single": dict(path="uniform"),
    "hot2": dict(path="hot", exit="drained", rounds=2, first=32, leftover=0),
    "hot8": dict(path="hot", exit="drained", rounds=8, first=8, leftover=0),
    "hot_then_tail": dict(path="hot", exit="rounds8", rounds=8, first=16,
                          leftover=41),
    "bail": dict(path="hot", exit="bail", rounds=1, first=7, leftover=57),
    "interleaved": dict(path="hot", exit="drained", rounds=2, first=32,
                        leftover=0),
    "scatter": dict(path="hot", exit="bail", rounds=1, first=1, leftover=63),
}


def simulate_wave(g):
    """CPU restatement of k_agg_update's per-wave path choice for the group
    ids of one 64-row slice (shorter = partial last wave)."""
    g = list(g)
    if len(g) == WAVE and len(set(g)) == 1:
        return dict(path="uniform")
    todo = list(range(len(g)))
    rounds, first, exit_ = 0, None, "drained"
    while todo and rounds < 8:
        gsel = g[todo[0]]
        mine = [l for l in todo if g[l] == gsel]
        todo = [l for l in todo if g[l] != gsel]
        rounds += 1
        if rounds == 1:
            first = len(mine)
            if first < 8:
                exit_ = "bail"
                break
    if todo and exit_ != "bail":
        exit_ = "rounds8"
    return dict(path="hot", exit=exit_, rounds=rounds, first=first,
                leftover=len(todo))


# streaming: clustered keys from run lengths
def runs_to_gids(lengths, n):
    """group index per row for runs of the given lengths, cycled to n rows"""
    out, r = [], 0
    total = 0
    while total < n:
        ln = lengths[r % len(lengths)]
        out.append(np.full(ln, r, np.int64))
        total += ln
        r += 1
    return np.concatenate(out)[:n]


STREAM_SHAPES = {
    # every row its own run: every lane is a run end
    "runs1": (1,),
    # runs one short of, equal to and one past a wave
    "runs63_64_65": (63, 64, 65),
    # one run of 200 spanning more than three waves, between short runs
    "run200": (10, 200, 7, 3),
    # cumulative ends 63, 64, 65, 128 (period 128): runs end exactly at
    # lanes 62, 63 and 0
    "ends62_63_0": (63, 1, 1, 63),
}


# --------------------------------------------------------------------------
# columns, pages
# --------------------------------------------------------------------------
class Col:
    def __init__(self, values, valid=None):
        self.values = np.ascontiguousarray(values)
        self.valid = None if valid is None else np.asarray(valid, bool)

    def ok(self):
        return (np.ones(len(self.values), bool) if self.valid is None
                else self.valid)


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


def make_page(ops, cols, lo, hi):
    arrs = [np.ascontiguousarray(c.values[lo:hi]) for c in cols]
    vals = [None if c.valid is None else pack_valid(c.valid[lo:hi])
            for c in cols]
    return ops.page_from_numpy(arrs, vals)


def feed(op, ops, cols, cuts=()):
    n = len(cols[0].values)
    edges = [0] + list(cuts) + [n]
    for lo, hi in zip(edges[:-1], edges[1:]):
        op.add_input(make_page(ops, cols, lo, hi))


def collect(op):
    """drain + close; concatenated output as [(values, valid_bool)]"""
    pages = op.drain()
    op.close()
    if not pages:
        return None
    out = []
    for c in range(len(pages[0])):
        vals = np.concatenate([np.asarray(p[c]["values"]) for p in pages])
        valid = np.concatenate([unpack_valid(p[c]["valid"], len(p[c]["values"]))
                                for p in pages])
        out.append((vals, valid))
    return out


def split_cut(ng):
    """cut that splits ng rows into two non-empty pages (none for one row)"""
    return () if ng < 2 else (max(1, ng // 3),)


def out_cols(out):
    """output page -> Col list (to feed a FINAL operator)"""
    return [Col(v, None if ok.all() else ok) for v, ok in out]


# --------------------------------------------------------------------------
# reference
# --------------------------------------------------------------------------
class Agg:
    def __init__(self, fn, ch=-1, scale_pow=0, mask=None):
        self.fn, self.ch, self.scale_pow, self.mask = fn, ch, scale_pow, mask

    def spec(self):
        if self.mask:
            return (self.fn, self.ch, self.scale_pow, self.mask[0], self.mask[1])
        return (self.fn, self.ch, self.scale_pow)


class Ref:
    def __init__(self, keys, cols, bounds, sizes):
        self.keys, self.cols, self.bounds, self.sizes = keys, cols, bounds, sizes


def to_i64(x):
    return (x + 2 ** 63) % 2 ** 64 - 2 ** 63


def _per_group(gid, ng, ok, vals, fn, empty=None):
    """fn(list of Python values of the ok rows) per group; `empty` where a
    group has none. Selection is numpy, the arithmetic is Python's."""
    idx = np.flatnonzero(ok)
    g = gid[idx]
    order = np.argsort(g, kind="stable")
    lst = vals[idx][order].tolist()
    ends = np.cumsum(np.bincount(g, minlength=ng)).tolist()
    starts = [0] + ends[:-1]
    return [fn(lst[a:b]) if b > a else empty for a, b in zip(starts, ends)]


def reference(cols, key_chs, aggs):
    n = len(cols[0].values)
    if key_chs:
        kl = []
        for c in key_chs:
            v = cols[c].values.tolist()
            if cols[c].valid is not None:
                v = [x if o else None for x, o in zip(v, cols[c].valid.tolist())]
            kl.append(v)
        ids = {}
        gid = np.fromiter((ids.setdefault(k, len(ids)) for k in zip(*kl)),
                          np.int64, n)
        keys = list(ids)
    else:
        gid, keys = np.zeros(n, np.int64), [()]
    ng = len(keys)
    sizes = np.bincount(gid, minlength=ng).tolist()
    rcols, rbounds = [], []
    for ag in aggs:
        ok = np.ones(n, bool)
        if ag.mask:
            a, b = cols[ag.mask[0]], cols[ag.mask[1]]
            ok = a.ok() & b.ok() & (a.values.astype(np.int64) >
                                    b.values.astype(np.int64))
        bound = None
        if ag.fn == COUNT_STAR:
            col = _per_group(gid, ng, ok, gid, len, 0)
        else:
            vc = cols[ag.ch]
            okv = ok & vc.ok()
            v = vc.values
            if ag.fn == COUNT_COL:
                col = _per_group(gid, ng, okv, v, len, 0)
            elif ag.fn == SUM_I64:
                col = _per_group(gid, ng, okv, v, lambda x: to_i64(sum(x)))
            elif ag.fn == MIN_I64:
                col = _per_group(gid, ng, okv, v, min)
            elif ag.fn == MAX_I64:
                col = _per_group(gid, ng, okv, v, max)
            elif ag.fn == SUM_F64_EXACT:
                assert_exact_precondition(v[okv], ag.scale_pow)
                col = _per_group(gid, ng, okv, v, math.fsum)
            else:
                sums = _per_group(gid, ng, okv, v, math.fsum)
                sabs = _per_group(gid, ng, okv, np.abs(v), math.fsum, 0.0)
                cnt = _per_group(gid, ng, okv, v, len, 0)
                sb = [ngr * U * s for ngr, s in zip(sizes, sabs)]
                if ag.fn == SUM_F64:
                    col, bound = sums, sb
                else:
                    col = [None if c == 0 else s / c for s, c in zip(sums, cnt)]
                    bound = [0.0 if c == 0 else b / c + U * abs(s / c)
                             for s, c, b in zip(sums, cnt, sb)]
        rcols.append(col)
        rbounds.append(bound)
    return Ref(keys, rcols, rbounds, sizes)


def assert_exact_precondition(v, scale_pow):
    """every v * 2^scale_pow is an integer below 2^63 in magnitude (scaling
    by a power of two is exact in f64)"""
    y = np.asarray(v, np.float64) * 2.0 ** scale_pow
    assert np.all(np.isfinite(y)) and np.all(y == np.floor(y))
    assert np.all(np.abs(y) < 2.0 ** 63)


def assert_sums_defined(ref, aggs):
    """outside the xfail: every group has a non-NULL addend for every SUM"""
    for ag, col in zip(aggs, ref.cols):
        if ag.fn in SUM_KINDS:
            assert all(x is not None for x in col)


def check(ref, out, key_dtypes, aggs, sort_keys=False):
    assert out is not None and len(out) == len(key_dtypes) + len(aggs)
    ng = len(ref.keys)
    perm = list(range(ng))
    if sort_keys:
        perm.sort(key=lambda i: ref.keys[i])
    for c, dt in enumerate(key_dtypes):
        exp = [ref.keys[i][c] for i in perm]
        ev = np.array([e is not None for e in exp], bool)
        evals = np.array([0 if e is None else e for e in exp], dt)
        got, gvalid = out[c]
        assert len(got) == ng, (len(got), ng)
        assert np.array_equal(gvalid, ev)
        assert np.array_equal(got[ev], evals[ev])
    for a, ag in enumerate(aggs):
        got, gvalid = out[len(key_dtypes) + a]
        exp = [ref.cols[a][i] for i in perm]
        assert len(got) == ng, (a, len(got), ng)
        ev = np.array([e is not None for e in exp], bool)
        assert np.array_equal(gvalid, ev), ("validity", a, ag.fn)
        if ag.fn in (SUM_F64, AVG_F64):
            e = np.array([0.0 if x is None else x for x in exp])
            b = np.array([ref.bounds[a][i] for i in perm])
            err = np.abs(got - e)
            assert np.all(err[ev] <= b[ev]), (a, ag.fn, float(np.max(err[ev] - b[ev])))
        elif ag.fn == SUM_F64_EXACT:
            e = np.array([0.0 if x is None else x for x in exp])
            assert np.array_equal(got[ev], e[ev]), ("exact", a)
        else:
            e = np.array([0 if x is None else x for x in exp], np.int64)
            assert np.array_equal(got[ev], e[ev]), ("int", a, ag.fn)


# --------------------------------------------------------------------------
# value patterns
# --------------------------------------------------------------------------
def first_rows(gid):
    first = np.zeros(len(gid), bool)
    first[np.unique(gid, return_index=True)[1]] = True
    return first


def value_cols(gid, seed, nulls=True):
    """[iv, fv, ew, em]: BIGINT over +-2^40; DOUBLE; exact 'wide' grid
    m*2^10/2^20 with 2^50 <= |m| < 2^52 (scale_pow 20; group sums cross 2^64
    in scaled units, both signs, > 53 significant bits); exact money grid
    (scale_pow 43). ~30 % NULLs, but each group's first row is non-NULL.
    NULL cells carry hostile data words."""
    r = rng(seed)
    n = len(gid)
    keep = first_rows(gid)

    def nullmask():
        if not nulls:
            return None
        return (r.random(n) >= 0.3) | keep

    iv = r.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    fv = r.standard_normal(n) * 1e6
    mostly = np.where(gid % 2 == 0, 0.8, 0.2)
    sign = np.where(r.random(n) < mostly, 1, -1).astype(np.int64)
    m = r.integers(2 ** 50, 2 ** 52, n, dtype=np.int64) * sign
    ew = m.astype(np.float64) / 1024.0
    em = r.integers(90100, 209900, n).astype(np.float64) / 100.0
    cols = []
    for v, poison in ((iv, POISON_I), (fv, np.nan), (ew, np.nan), (em, np.nan)):
        ok = nullmask()
        if ok is not None:
            v = v.copy()
            v[~ok] = poison
        cols.append(Col(v, ok))
    return cols


def all_aggs(base):
    """the eight kinds (+ the second exact grid) over value_cols at `base`"""
    return [Agg(COUNT_STAR), Agg(COUNT_COL, base), Agg(SUM_F64, base + 1),
            Agg(SUM_I64, base), Agg(AVG_F64, base + 1),
            Agg(SUM_F64_EXACT, base + 2, SP_WIDE), Agg(MIN_I64, base),
            Agg(MAX_I64, base), Agg(SUM_F64_EXACT, base + 3, SP_MONEY)]


def final_aggs(aggs, nk):
    """agg specs of the FINAL step over a PARTIAL output page"""
    out, ch = [], nk
    for ag in aggs:
        out.append(Agg(ag.fn, ch, ag.scale_pow))
        ch += 2 if ag.fn in (AVG_F64, SUM_F64_EXACT) else 1
    return out


KEYFORMS = {"bigint": 1, "two_channel": 2, "scalar": 0}


@functools.lru_cache(maxsize=None)
def hash_case(shape, n, keyform):
    """(cols, key channels, key dtypes, aggs, reference), computed once and
    shared by the tests that run this input; never modified."""
    gid = np.asarray(SHAPES[shape](n), np.int64)
    nk = KEYFORMS[keyform]
    if nk == 2:
        keys = [Col(key_of(gid >> 1)),
                Col(np.where(gid & 1, -7, 2_000_000_000).astype(np.int32))]
    else:
        keys = [Col(key_of(gid))] if nk == 1 else []
    vg = gid if nk else np.zeros(n, np.int64)
    cols = keys + value_cols(vg, 1000 + n)
    aggs = all_aggs(nk)
    ref = reference(cols, list(range(nk)), aggs)
    assert_sums_defined(ref, aggs)
    dts = [np.int64, np.int32][:nk]
    return cols, list(range(nk)), dts, aggs, ref


def hash_op(ops, sess, key_chs, dts, aggs, step=SINGLE):
    tys = [ops.TG_BIGINT if d == np.int64 else ops.TG_INTEGER for d in dts]
    return ops.hash_aggregation(sess, key_chs, tys, [a.spec() for a in aggs],
                                step=step)


def run_hash(ops, sess, cols, key_chs, dts, aggs, cuts=(), step=SINGLE):
    op = hash_op(ops, sess, key_chs, dts, aggs, step)
    feed(op, ops, cols, cuts)
    return collect(op)


# --------------------------------------------------------------------------
# hash aggregation
# --------------------------------------------------------------------------
HASH_CASES = ([(s, n, "bigint") for s in SHAPES for n in SMALL_NS] +
              [(s, 1000, "two_channel") for s in SHAPES] +
              [("single", n, "scalar") for n in SMALL_NS])


@pytest.mark.parametrize("shape,n,keyform", HASH_CASES)
def test_hash_single(sess, ops, shape, n, keyform):
    cols, kc, dts, aggs, ref = hash_case(shape, n, keyform)
    check(ref, run_hash(ops, sess, cols, kc, dts, aggs), dts, aggs)


@pytest.mark.parametrize("cuts", [(64,), (64, 65)], ids=["2pages", "3pages"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_hash_page_splits(sess, ops, shape, cuts):
    cols, kc, dts, aggs, ref = hash_case(shape, 1000, "bigint")
    check(ref, run_hash(ops, sess, cols, kc, dts, aggs, cuts), dts, aggs)


@pytest.mark.parametrize("shape,keyform",
                         [(s, "bigint") for s in SHAPES] +
                         [("hot8", "two_channel"), ("single", "scalar")])
def test_hash_partial_final(sess, ops, shape, keyform):
    """PARTIAL over two input pages, then FINAL fed the PARTIAL page split in
    two (cut at 1/3 of the groups; a single group cannot be split)."""
    cols, kc, dts, aggs, ref = hash_case(shape, 1000, keyform)
    part = run_hash(ops, sess, cols, kc, dts, aggs, (500,), PARTIAL)
    pcols = out_cols(part)
    ng = len(pcols[0].values)
    assert ng == len(ref.keys)
    faggs = final_aggs(aggs, len(kc))
    out = run_hash(ops, sess, pcols, kc, dts, faggs, split_cut(ng), FINAL)
    check(ref, out, dts, aggs)


def test_hash_grid_stride(sess, ops):
    """n = 524288 + 64*3 + 5: the stride loop of k_gt_assign and k_agg_update
    iterates twice; the second pass has three full waves and a 5-row one."""
    cols, kc, dts, aggs, ref = hash_case("hot_then_tail", GRID_STRIDE_N, "bigint")
    assert GRID_STRIDE_N > GRID_THREADS and GRID_STRIDE_N % WAVE == 5
    check(ref, run_hash(ops, sess, cols, kc, dts, aggs), dts, aggs)


def test_hash_sum_i64_wraps_mod_2_64(sess, ops):
    """two addends whose sum passes 2^63: two's-complement wraparound equals
    Python's sum reduced mod 2^64 (hash, streaming and dense)."""
    k = np.array([5, 5, 9, 9, 9], np.int64)
    v = np.array([2 ** 62 + 5, 2 ** 62 + 7, -2 ** 62, -2 ** 62, -2 ** 62], np.int64)
    cols = [Col(k), Col(v)]
    aggs = [Agg(SUM_I64, 1)]
    ref = reference(cols, [0], aggs)
    assert ref.cols[0] == [-2 ** 63 + 12, 2 ** 62]
    check(ref, run_hash(ops, sess, cols, [0], [np.int64], aggs), [np.int64], aggs)
    op = ops.streaming_aggregation(sess, 0, [a.spec() for a in aggs])
    feed(op, ops, cols)
    check(ref, collect(op), [np.int64], aggs)
    op = ops.dense_aggregation(sess, 0, 5, 9, aggs[0].spec())
    feed(op, ops, cols)
    check(ref, collect(op), [np.int64], aggs, sort_keys=True)


def null_group_cols():
    """3 groups x 70 rows, interleaved; group 1's value cells are all NULL"""
    gid = np.arange(210, dtype=np.int64) % 3
    cols = [Col(key_of(gid))] + value_cols(gid, 77)
    for c in cols[1:]:
        c.valid = c.valid & (gid != 1)
        c.values[gid == 1] = c.values[gid == 1] * 0 + (
            POISON_I if c.values.dtype == np.int64 else np.nan)
    return gid, cols


NULL_GROUP_AGGS = [Agg(COUNT_STAR), Agg(COUNT_COL, 1), Agg(MIN_I64, 1),
                   Agg(MAX_I64, 1), Agg(AVG_F64, 2)]


@pytest.mark.parametrize("operator", ["hash", "hash_partial_final", "streaming"])
def test_all_null_group_is_null(sess, ops, operator):
    """a group whose values are all NULL: COUNT_COL 0, MIN/MAX/AVG NULL"""
    gid, cols = null_group_cols()
    if operator == "streaming":
        order = np.argsort(gid, kind="stable")
        cols = [Col(c.values[order], c.valid if c.valid is None else c.valid[order])
                for c in cols]
    ref = reference(cols, [0], NULL_GROUP_AGGS)
    assert ref.cols[1][1] == 0 and ref.cols[2][1] is None and ref.cols[4][1] is None
    if operator == "hash":
        out = run_hash(ops, sess, cols, [0], [np.int64], NULL_GROUP_AGGS, (100,))
    elif operator == "hash_partial_final":
        part = run_hash(ops, sess, cols, [0], [np.int64], NULL_GROUP_AGGS,
                        (100,), PARTIAL)
        out = run_hash(ops, sess, out_cols(part), [0], [np.int64],
                       final_aggs(NULL_GROUP_AGGS, 1), (1,), FINAL)
    else:
        op = ops.streaming_aggregation(sess, 0, [a.spec() for a in NULL_GROUP_AGGS])
        feed(op, ops, cols, (100,))
        out = collect(op)
    check(ref, out, [np.int64], NULL_GROUP_AGGS)


@pytest.mark.xfail(strict=True, raises=AssertionError, reason="recorded deviation: SUM_I64 / SUM_F64 / "
                   "SUM_F64_EXACT over a group with no non-NULL input emit 0 "
                   "without a validity bitmap where SQL says NULL")
def test_sum_of_no_input_is_null(sess, ops):
    _, cols = null_group_cols()
    aggs = [Agg(SUM_I64, 1), Agg(SUM_F64, 2), Agg(SUM_F64_EXACT, 4, SP_MONEY)]
    ref = reference(cols, [0], aggs)
    assert all(c[1] is None for c in ref.cols)
    check(ref, run_hash(ops, sess, cols, [0], [np.int64], aggs), [np.int64], aggs)


SCALAR_EMPTY_AGGS = [Agg(COUNT_STAR), Agg(COUNT_COL, 0), Agg(MIN_I64, 0),
                     Agg(MAX_I64, 0), Agg(AVG_F64, 1)]


@pytest.mark.parametrize("pages", ["no_page", "one_empty_page"])
@pytest.mark.parametrize("step", [SINGLE, FINAL], ids=["single", "final"])
def test_scalar_aggregation_of_nothing_emits_one_row(sess, ops, step, pages):
    """no group channels: exactly one row, COUNT 0 and MIN/MAX/AVG NULL"""
    if step == FINAL:    # partial layout: count, count, min, max, (count, sum)
        cols = [Col(np.zeros(0, np.int64)) for _ in range(5)] + [Col(np.zeros(0))]
        aggs = final_aggs(SCALAR_EMPTY_AGGS, 0)
    else:
        cols = [Col(np.zeros(0, np.int64)), Col(np.zeros(0))]
        aggs = SCALAR_EMPTY_AGGS
    ref = reference([Col(np.zeros(0, np.int64)), Col(np.zeros(0))], [],
                    SCALAR_EMPTY_AGGS)
    assert ref.keys == [()] and ref.cols == [[0], [0], [None], [None], [None]]
    op = hash_op(ops, sess, [], [], aggs, step)
    if pages == "one_empty_page":
        feed(op, ops, cols)
    check(ref, collect(op), [], SCALAR_EMPTY_AGGS)


# --------------------------------------------------------------------------
# masks (hash and streaming)
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mask_case():
    """clustered keys (valid for both operators). Channels: key, value,
    INTEGER mask pair (every group has a passing row with a non-NULL value, so
    the masked SUM is defined), BIGINT mask pair (groups 0 mod 4 have no
    passing row). Both pairs carry negatives and ~25 % NULLs whose data words
    would pass the gate if read."""
    n = 1500
    gid = runs_to_gids((5, 70, 1, 64, 9), n)
    r = rng(91)
    first = first_rows(gid)
    iv = r.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    iv_ok = (r.random(n) >= 0.3) | first
    iv[~iv_ok] = POISON_I
    a32 = r.integers(-50, 50, n).astype(np.int32)
    b32 = r.integers(-50, 50, n).astype(np.int32)
    a32[first], b32[first] = 5, -5
    a32_ok = (r.random(n) >= 0.25) | first
    b32_ok = (r.random(n) >= 0.25) | first
    a32[~a32_ok], b32[~b32_ok] = 2 ** 31 - 1, -2 ** 31
    a64 = r.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    b64 = r.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    dead = gid % 4 == 0
    a64[dead] = b64[dead] - r.integers(0, 3, int(dead.sum()))
    a64_ok = r.random(n) >= 0.25
    b64_ok = r.random(n) >= 0.25
    a64[~a64_ok], b64[~b64_ok] = 2 ** 62, -2 ** 62
    cols = [Col(key_of(gid)), Col(iv, iv_ok), Col(a32, a32_ok), Col(b32, b32_ok),
            Col(a64, a64_ok), Col(b64, b64_ok)]
    kinds = (COUNT_STAR, SUM_I64, MIN_I64, MAX_I64)
    aggs = ([Agg(f, 1 if f != COUNT_STAR else -1) for f in kinds] +
            [Agg(f, 1 if f != COUNT_STAR else -1, 0, (2, 3)) for f in kinds] +
            [Agg(f, 1 if f != COUNT_STAR else -1, 0, (4, 5))
             for f in (COUNT_STAR, MIN_I64, MAX_I64)])
    ref = reference(cols, [0], aggs)
    assert_sums_defined(ref, aggs)
    # some groups have no passing row (masked COUNT 0, MIN/MAX NULL)
    assert 0 in ref.cols[8] and None in ref.cols[9] and None in ref.cols[10]
    assert any(x is not None for x in ref.cols[9])
    return cols, aggs, ref


@pytest.mark.parametrize("operator", ["hash", "streaming"])
def test_masked_aggregates(sess, ops, operator):
    cols, aggs, ref = mask_case()
    if operator == "hash":
        out = run_hash(ops, sess, cols, [0], [np.int64], aggs, (700,))
    else:
        op = ops.streaming_aggregation(sess, 0, [a.spec() for a in aggs])
        feed(op, ops, cols, (700,))
        out = collect(op)
    check(ref, out, [np.int64], aggs)


# --------------------------------------------------------------------------
# streaming aggregation
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream_case(shape, n):
    lengths = STREAM_SHAPES[shape] if isinstance(shape, str) else shape
    gid = runs_to_gids(lengths, n)
    cols = [Col(key_of(gid))] + value_cols(gid, 2000 + n)
    aggs = all_aggs(1)
    ref = reference(cols, [0], aggs)
    assert_sums_defined(ref, aggs)
    return gid, cols, aggs, ref


def run_stream(ops, sess, cols, aggs, cuts=(), step=SINGLE):
    op = ops.streaming_aggregation(sess, 0, [a.spec() for a in aggs], step=step)
    feed(op, ops, cols, cuts)
    return collect(op)


def stream_cuts(gid):
    """one cut at a run boundary near n/3, one mid-run near 2n/3 (if any)"""
    n = len(gid)
    starts = np.flatnonzero(np.diff(gid)) + 1
    mids = np.setdiff1d(np.arange(1, n), starts)
    cuts = {int(starts[np.searchsorted(starts, n // 3)])}
    if len(mids):
        cuts.add(int(mids[min(np.searchsorted(mids, 2 * n // 3), len(mids) - 1)]))
    return tuple(sorted(cuts))


@pytest.mark.parametrize("step", [SINGLE, PARTIAL], ids=["single", "partial"])
@pytest.mark.parametrize("n", SMALL_NS)
@pytest.mark.parametrize("shape", list(STREAM_SHAPES))
def test_streaming(sess, ops, shape, n, step):
    """SINGLE against the reference; PARTIAL states through a hash FINAL"""
    gid, cols, aggs, ref = stream_case(shape, n)
    out = run_stream(ops, sess, cols, aggs, (), step)
    if step == PARTIAL:
        out = run_hash(ops, sess, out_cols(out), [0], [np.int64],
                       final_aggs(aggs, 1), split_cut(len(ref.keys)), FINAL)
    check(ref, out, [np.int64], aggs)


@pytest.mark.parametrize("shape", list(STREAM_SHAPES))
def test_streaming_page_cuts(sess, ops, shape):
    gid, cols, aggs, ref = stream_case(shape, 1000)
    cuts = stream_cuts(gid)
    starts = set((np.flatnonzero(np.diff(gid)) + 1).tolist())
    assert any(c in starts for c in cuts)
    if shape != "runs1":
        assert any(c not in starts for c in cuts)
    check(ref, run_stream(ops, sess, cols, aggs, cuts), [np.int64], aggs)


def test_streaming_grid_stride(sess, ops):
    gid, cols, aggs, ref = stream_case((4159, 4160, 4161, 1), GRID_STRIDE_N)
    check(ref, run_stream(ops, sess, cols, aggs), [np.int64], aggs)


def test_streaming_nullable_key_unsupported(sess, ops):
    import trino_amd
    k = np.arange(10, dtype=np.int64)
    op = ops.streaming_aggregation(sess, 0, [(COUNT_STAR, -1)])
    with pytest.raises(trino_amd.TrinoGpuError):
        op.add_input(make_page(ops, [Col(k, k != 3)], 0, 10))
    op.close()


# --------------------------------------------------------------------------
# state growth with live MIN/MAX state
# --------------------------------------------------------------------------
GROWTH_AGGS = [Agg(MIN_I64, 1), Agg(MAX_I64, 1), Agg(SUM_I64, 1),
               Agg(SUM_F64_EXACT, 2, SP_MONEY)]


def growth_values(gid, seed):
    r = rng(seed)
    n = len(gid)
    iv = r.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    em = r.integers(90100, 209900, n).astype(np.float64) / 100.0
    return [Col(iv), Col(em)]


def assert_page2_moves_min_max(cols, cut, ref):
    """some page-1 groups get a new MIN and some a new MAX from page 2"""
    head = [Col(c.values[:cut]) for c in cols]
    r1 = reference(head, [0], GROWTH_AGGS[:2])
    n1 = len(r1.keys)
    assert ref.keys[:n1] == r1.keys
    assert any(a != b for a, b in zip(r1.cols[0], ref.cols[0][:n1]))
    assert any(a != b for a, b in zip(r1.cols[1], ref.cols[1][:n1]))


def test_hash_growth_with_live_state(sess, ops):
    """60,000 distinct keys, then 20,000 rows half of them new keys:
    HashAggOp::grow_if_needed crosses max_groups = 65,536 with MIN (0xFF
    identity) / MAX / SUM / exact state populated."""
    r = rng(5)
    g1 = r.permutation(60_000)
    g2 = r.permutation(np.concatenate([np.arange(60_000, 70_000),
                                       r.choice(60_000, 10_000, replace=False)]))
    gid = np.concatenate([g1, g2]).astype(np.int64)
    cols = [Col(key_of(gid))] + growth_values(gid, 6)
    ref = reference(cols, [0], GROWTH_AGGS)
    assert len(ref.keys) == 70_000 > 65_536 > 60_000
    assert_page2_moves_min_max(cols, 60_000, ref)
    out = run_hash(ops, sess, cols, [0], [np.int64], GROWTH_AGGS, (60_000,))
    check(ref, out, [np.int64], GROWTH_AGGS)


def test_streaming_growth_with_live_state(sess, ops):
    """60,000 runs, then 10,000 more (page 2 opens by continuing page 1's last
    run): StreamAggOp::ensure_runs crosses runs_cap = 65,536 with live state."""
    r = rng(7)
    len1 = np.where(r.random(60_000) < 0.08, 2, 1)
    len1[-1] = 3
    len2 = np.where(r.random(10_000) < 0.2, 2, 1)
    g1 = np.repeat(np.arange(60_000), len1)
    g2 = np.concatenate([np.full(40, 59_999), np.repeat(np.arange(60_000, 70_000), len2)])
    gid = np.concatenate([g1, g2]).astype(np.int64)
    assert len(gid) <= 80_000
    cols = [Col(key_of(gid))] + growth_values(gid, 8)
    ref = reference(cols, [0], GROWTH_AGGS)
    assert len(ref.keys) == 70_000
    head = reference([Col(c.values[:len(g1)]) for c in cols], [0], GROWTH_AGGS[:2])
    assert (head.cols[0][-1], head.cols[1][-1]) != (ref.cols[0][59_999], ref.cols[1][59_999])
    out = run_stream(ops, sess, cols, GROWTH_AGGS, (len(g1),))
    check(ref, out, [np.int64], GROWTH_AGGS)


# --------------------------------------------------------------------------
# dense-range aggregation
# --------------------------------------------------------------------------
DENSE_FNS = {"count_star": COUNT_STAR, "count_col": COUNT_COL,
             "sum_i64": SUM_I64, "sum_exact": SUM_F64_EXACT}
# update kernel by (state words, range): 1 word: LDS <= 8192 < global;
# 2 words (exact): LDS <= 4096 < global
DENSE_RANGES = (1, 64, 4096, 4097, 8192, 8193)


def dense_agg(fn):
    if fn == COUNT_STAR:
        return Agg(COUNT_STAR)
    if fn == SUM_F64_EXACT:
        return Agg(fn, 1, SP_WIDE)
    return Agg(fn, 1)


def dense_reference(cols, key_min, key_max, agg):
    """reference over the rows whose key is non-NULL and in range"""
    k = cols[0]
    keep = k.ok() & (k.values >= key_min) & (k.values <= key_max)
    kept = [Col(c.values[keep].astype(np.int64) if c is k else c.values[keep],
                None if c.valid is None or c is k else c.valid[keep])
            for c in cols]
    ref = reference(kept, [0], [agg])
    assert_sums_defined(ref, [agg])
    return ref


def dense_cols(n, key_min, rng_size, fn, key_dtype, seed):
    """keys uniform over the range with ~10 % NULL keys; values with NULLs
    (each key's first row non-NULL). Three keys get a zero state: one whose
    integers / exact addends cancel, one whose values are NULL except a 0,
    and for COUNT_COL one whose values are all NULL."""
    r = rng(seed)
    kpos = r.integers(0, rng_size, n).astype(np.int64)
    k_ok = r.random(n) >= 0.1
    v_int = r.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    sign = np.where(r.random(n) < np.where(kpos % 2 == 0, 0.8, 0.2), 1, -1)
    v_f = (r.integers(2 ** 50, 2 ** 52, n, dtype=np.int64) * sign).astype(np.float64) / 1024.0
    exact = fn == SUM_F64_EXACT
    v = v_f if exact else v_int
    v_ok = (r.random(n) >= 0.3) | first_rows(np.where(k_ok, kpos, -1))
    # zero-state keys (positions 0 and, when the range has them, 1 and 2)
    z = np.flatnonzero(k_ok & (kpos == 0))
    v_ok[z] = True
    if len(z) % 2:
        v[z[-1]] = 0
    z = z[:len(z) // 2 * 2]
    v[z[1::2]] = -v[z[0::2]]
    if rng_size > 2:
        z = np.flatnonzero(k_ok & (kpos == 1))
        if len(z):
            v_ok[z] = False
            v[z[0]], v_ok[z[0]] = 0, True
        if fn == COUNT_COL:
            v_ok[k_ok & (kpos == 2)] = False
    v[~v_ok] = np.nan if exact else POISON_I
    keys = (kpos + key_min).astype(key_dtype)
    keys[~k_ok] = key_min          # in-range data word under the NULL key
    return [Col(keys, k_ok), Col(v, v_ok)]


def run_dense(ops, sess, cols, key_min, key_max, agg, cuts=()):
    op = ops.dense_aggregation(sess, 0, key_min, key_max, agg.spec())
    feed(op, ops, cols, cuts)
    return collect(op)


@pytest.mark.parametrize("key_dtype", [np.int64, np.int32], ids=["bigint", "integer"])
@pytest.mark.parametrize("rng_size", DENSE_RANGES)
@pytest.mark.parametrize("fname", list(DENSE_FNS))
def test_dense(sess, ops, fname, rng_size, key_dtype):
    """every update kernel for both state widths; key_min negative for the
    INTEGER-keyed cases; NULL keys dropped; zero-state keys still emitted;
    two pages so state carries across launches."""
    fn = DENSE_FNS[fname]
    key_min = -(rng_size // 2) - 3 if key_dtype == np.int32 else 7
    key_max = key_min + rng_size - 1
    n = 20_000
    cols = dense_cols(n, key_min, rng_size, fn, key_dtype, 300 + rng_size)
    agg = dense_agg(fn)
    ref = dense_reference(cols, key_min, key_max, agg)
    if fn in (SUM_I64, SUM_F64_EXACT) or (fn == COUNT_COL and rng_size > 2):
        assert 0 in ref.cols[0]          # a present key whose state is zero
    out = run_dense(ops, sess, cols, key_min, key_max, agg, (9_999,))
    check(ref, out, [np.int64], [agg], sort_keys=True)


@pytest.mark.parametrize("rng_size", [16_384, 16_385])
@pytest.mark.parametrize("fname", ["count_star", "sum_i64", "sum_exact"])
def test_dense_emit_chunk_edges(sess, ops, fname, rng_size):
    """keys only at positions 0, 63, 64, 16383 (and 16384 when in range):
    ballot / offset arithmetic of k_dense_emit and k_dense_emit_exact at
    64-lane and 16384-entry chunk edges."""
    fn = DENSE_FNS[fname]
    pos = [p for p in (0, 63, 64, 16_383, 16_384) if p < rng_size]
    key_min = -100
    k = np.repeat(np.array(pos, np.int64) + key_min, 3)
    v = (np.arange(len(k)) - 4) * 3
    cols = [Col(k), Col(v.astype(np.float64) if fn == SUM_F64_EXACT
                        else v.astype(np.int64))]
    agg = dense_agg(fn)
    ref = dense_reference(cols, key_min, key_min + rng_size - 1, agg)
    assert len(ref.keys) == len(pos)
    out = run_dense(ops, sess, cols, key_min, key_min + rng_size - 1, agg)
    check(ref, out, [np.int64], [agg], sort_keys=True)


@pytest.mark.parametrize("fname", ["sum_i64", "sum_exact"])
def test_dense_out_of_range_keys_dropped(sess, ops, fname):
    """keys below key_min and above key_max are dropped; in-range results are
    what they are without those rows"""
    fn = DENSE_FNS[fname]
    r = rng(41)
    n = 5_000
    k = r.integers(-40, 140, n).astype(np.int64)      # range is [0, 99]
    k[:4] = [-1, 100, 0, 99]
    v = r.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    cols = [Col(k), Col(v.astype(np.float64) if fn == SUM_F64_EXACT else v)]
    agg = dense_agg(fn)
    ref = dense_reference(cols, 0, 99, agg)
    assert len(ref.keys) == 100 and np.any(k < 0) and np.any(k > 99)
    check(ref, run_dense(ops, sess, cols, 0, 99, agg), [np.int64], [agg],
          sort_keys=True)


@pytest.mark.parametrize("fname,rng_size", [("count_col", 64), ("sum_exact", 4097)])
def test_dense_grid_stride(sess, ops, fname, rng_size):
    """stride loop of the LDS kernel (1 word) and the global kernel (2 words)"""
    fn = DENSE_FNS[fname]
    cols = dense_cols(GRID_STRIDE_N, 7, rng_size, fn, np.int64, 55)
    agg = dense_agg(fn)
    ref = dense_reference(cols, 7, 6 + rng_size, agg)
    check(ref, run_dense(ops, sess, cols, 7, 6 + rng_size, agg), [np.int64],
          [agg], sort_keys=True)
