"""Q1 over the integer column forms: generator, dispatch, loop, decode, carries.

`tg_q1_run` scans quantity_u8 / extendedprice_cents / discount_pct / tax_pct
(13 B/row with shipdate and the two flag bytes) when all four pointers are set
and the f64 columns otherwise; both must give the same 60 result words. Every
comparison here is exact equality: the sums are error-free fixed point.

The reference is `oracle.q1_exact` on host f64 arrays derived from the integer
arrays in numpy — `k.astype(np.float64) / 100.0` and `q.astype(np.float64)`,
IEEE division, the generator's own expression. Hand-built columns are uploaded
the way test_gpu_q1_fused_matrix.py does; each integer column has its f64 twin
on the device, so every LineitemCols keeps the contract of trino_gpu.h.

One pool of rows per column variant is uploaded once; a case of n rows runs on
the first n rows (row_count = n) and the oracle on the same prefix.
"""
import os
import re

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

_Q1_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "trino_amd", "csrc", "q1.hip")


def _source_constant(name):
    with open(_Q1_SRC) as f:
        (m,) = re.findall(r"^#define %s (\d+)\b" % name, f.read(), re.M)
    return int(m)


# the integer kernel takes R rows per lane per iteration on at most GRID_CAP
# blocks of 256 lanes: a lane runs a second (pipelined) iteration once n > FULL
R = _source_constant("Q1I_R")
GRID_CAP = _source_constant("Q1I_GRID_CAP")
FULL = GRID_CAP * 256 * R
MAX_CENTS = 10_494_950                   # 50 x the dearest part, in cents
DOMAIN_N = MAX_CENTS + 1
LOOP_N = 2 * FULL + R                    # longest loop-boundary case + 1
CUT_HALF = 10000                         # shipdate is uniform in [8000, 12000)
CUT_NONE = 0
CUT_ALL = 1 << 30

SIZES = [0, 1, R - 1, R, R + 1, 255, 1024, 1025,
         FULL - 1, FULL, FULL + 1, FULL + R, FULL + R + 1,
         2 * FULL, 2 * FULL + 1, 2 * FULL + R - 1]

INT_FIELDS = ("quantity_u8", "extendedprice_cents", "discount_pct", "tax_pct")
# integer field -> (its f64 field, divisor)
F64_OF = dict(quantity_u8=("quantity", None), extendedprice_cents=("extendedprice", 100.0),
              discount_pct=("discount", 100.0), tax_pct=("tax", 100.0))


def decode(field, a):
    """the f64 column an integer column stands for"""
    div = F64_OF[field][1]
    x = a.astype(np.float64)
    return x if div is None else x / div


def assert_q1_equal(gpu, ora):
    for c in range(6):
        assert gpu.count[c] == ora.count[c], ("count", c, gpu.count[c], ora.count[c])
        assert gpu.sum_qty[c] == ora.sum_qty[c], ("sum_qty", c, gpu.sum_qty[c], ora.sum_qty[c])
        assert gpu.sum_base[c] == ora.sum_base[c], ("sum_base", c, gpu.sum_base[c], ora.sum_base[c])
        assert gpu.sum_disc_price[c] == ora.sum_disc_price[c], ("sum_disc_price", c)
        assert gpu.sum_charge[c] == ora.sum_charge[c], ("sum_charge", c)
        assert gpu.sum_disc[c] == ora.sum_disc[c], ("sum_disc", c)
        if ora.count[c]:
            assert gpu.avg_qty[c] == ora.avg_qty[c], ("avg_qty", c)
            assert gpu.avg_price[c] == ora.avg_price[c], ("avg_price", c)
            assert gpu.avg_disc[c] == ora.avg_disc[c], ("avg_disc", c)


def without(cols, *fields):
    """a copy of the struct with the named pointers zeroed"""
    import trino_amd
    c = trino_amd.LineitemCols.from_buffer_copy(cols)
    for f in fields:
        setattr(c, f, None)
    return c


# ------------------------------------------------------------ generated data

@pytest.fixture(scope="module")
def sess():
    import trino_amd
    s = trino_amd.Session(0)
    yield s
    s.close()


def _int_columns_to_host(sess, cols):
    import trino_amd
    n = cols.row_count
    out = {}
    for f, dt in zip(INT_FIELDS, (np.uint8, np.int32, np.uint8, np.uint8)):
        assert getattr(cols, f), f"{f} not generated"
        out[f] = trino_amd.copy_dtoh(sess, np.empty(n, dt), getattr(cols, f))
    return out


@pytest.mark.parametrize("sf,start,count", [
    (0.01, 1, 15000),        # full sf0.01
    (1.0, 700_001, 5000),    # mid-table part
    (1.0, 1_499_001, 1000),  # table tail
])
def test_generator_integer_columns(sess, sf, start, count):
    """the integer columns decode to the oracle's f64 columns and to the
    device's own, bit for bit"""
    import trino_amd
    cols = sess.tpch_lineitem(sf, start, count)
    ints = _int_columns_to_host(sess, cols)
    dev = trino_amd.lineitem_to_host(sess, cols)
    ref = oracle.gen_lineitem(sf, start, count)
    assert cols.row_count == len(ref["shipdate"])
    for f in INT_FIELDS:
        got = decode(f, ints[f])
        assert np.array_equal(got, ref[F64_OF[f][0]]), f
        assert np.array_equal(got, dev[F64_OF[f][0]]), f
    sess.tpch_lineitem_free(cols)


@pytest.mark.parametrize("sf,count", [(1.0, 1), (1.0, 2), (1.0, 3), (1.0, 63),
                                      (1.0, 64), (1.0, 1000), (0.01, 15000)])
def test_integer_path_equals_f64_path(sess, sf, count):
    cols = sess.tpch_lineitem(sf, 1, count)
    assert all(getattr(cols, f) for f in INT_FIELDS)
    gi = sess.q1(cols)
    gf = sess.q1(without(cols, *INT_FIELDS))
    ref, _ = oracle.q1_exact(oracle.gen_lineitem(sf, 1, count))
    assert list(gi.raw) == list(gf.raw)
    assert_q1_equal(gi, ref)
    assert_q1_equal(gf, ref)
    sess.tpch_lineitem_free(cols)


@pytest.mark.parametrize("missing", INT_FIELDS)
def test_partial_set_reads_f64(sess, missing):
    """all four or none: with one pointer NULL the scan reads the f64 columns"""
    cols = sess.tpch_lineitem(0.01)
    ref, _ = oracle.q1_exact(oracle.gen_lineitem(0.01))
    assert_q1_equal(sess.q1(without(cols, missing)), ref)
    sess.tpch_lineitem_free(cols)


# ------------------------------------------------------------ hand-built data

def _host_pool():
    """integer column variants (seeded); the f64 twins are derived on upload"""
    rng = np.random.default_rng(20261)
    n = LOOP_N
    h = {}
    h["shipdate"] = rng.integers(8000, 12000, DOMAIN_N, dtype=np.int32)
    # all six combos in random order, A|O and R|O included
    h["returnflag"] = rng.integers(0, 3, DOMAIN_N, dtype=np.uint8)
    h["linestatus"] = rng.integers(0, 2, DOMAIN_N, dtype=np.uint8)
    h["quantity_u8"] = rng.integers(1, 51, n, dtype=np.uint8)
    h["extendedprice_cents"] = rng.integers(0, MAX_CENTS + 1, n, dtype=np.int32)
    h["discount_pct"] = rng.integers(0, 11, n, dtype=np.uint8)
    h["tax_pct"] = rng.integers(0, 9, n, dtype=np.uint8)
    # variants
    h["rf_single"] = np.full(n, 2, np.uint8)        # every row R|O
    h["ls_single"] = np.full(n, 1, np.uint8)
    one = np.full(n, 11999, np.int32)               # one lane-row selected
    one[1_234_567] = 9000
    h["shipdate_one"] = one
    # decode domain: every price in cents once, the bytes cycling
    i = np.arange(DOMAIN_N, dtype=np.int64)
    h["cents_domain"] = i.astype(np.int32)
    h["qty_domain"] = (i % 50 + 1).astype(np.uint8)
    h["dpct_domain"] = (i % 11).astype(np.uint8)
    h["tpct_domain"] = (i % 9).astype(np.uint8)
    # addends near 2^62.7 (880,000.00 .. 900,000.00; charge * 2^43 < 2^63 at
    # tax 0.08): two same-combo rows wrap a lane's low 64 bits
    h["cents_big"] = rng.integers(88_000_000, 90_000_001, n, dtype=np.int32)
    h["rf_two"] = rng.integers(0, 2, n, dtype=np.uint8)   # combos A|F, N|F only
    h["ls_zero"] = np.zeros(n, np.uint8)
    # the byte columns' whole range
    h["qty_wide"] = rng.integers(0, 256, 1025, dtype=np.uint8)
    h["qty_wide"][:2] = (255, 0)
    dset = np.array(list(range(11)) + [99, 100], np.uint8)
    h["dpct_wide"] = dset[rng.integers(0, len(dset), 1025)]
    h["dpct_wide"][:2] = (100, 99)
    return h


_KIND = dict(quantity_u8="quantity_u8", qty_domain="quantity_u8", qty_wide="quantity_u8",
             extendedprice_cents="extendedprice_cents", cents_domain="extendedprice_cents",
             cents_big="extendedprice_cents",
             discount_pct="discount_pct", dpct_domain="discount_pct", dpct_wide="discount_pct",
             tax_pct="tax_pct", tpct_domain="tax_pct")


class _Pool:
    def __init__(self, sess):
        import trino_amd
        from trino_amd import tpch_queries as tq
        self.sess, self.tq, self.trino_amd = sess, tq, trino_amd
        self.host = {k: np.ascontiguousarray(a) for k, a in _host_pool().items()}
        # f64 twin of every integer column variant, under "<key>/f64"
        for k, field in _KIND.items():
            self.host[k + "/f64"] = decode(field, self.host[k])
        self.dev = {}
        for k, a in self.host.items():
            p = tq._device_buffer(sess, a.nbytes)
            trino_amd._check(trino_amd._lib.tg_copy_htod(sess._h, p, a.ctypes.data, a.nbytes))
            self.dev[k] = p
        self._ref = {}

    def close(self):
        for p in self.dev.values():
            self.tq._device_free(self.sess, p)

    def _names(self, over):
        names = dict(shipdate="shipdate", returnflag="returnflag", linestatus="linestatus",
                     quantity_u8="quantity_u8", extendedprice_cents="extendedprice_cents",
                     discount_pct="discount_pct", tax_pct="tax_pct")
        names.update(over)
        for f in INT_FIELDS:                       # the f64 twins follow
            names[F64_OF[f][0]] = names[f] + "/f64"
        return names

    def cols(self, n, **over):
        cols = self.trino_amd.LineitemCols()
        cols.row_count = n
        for field, key in self._names(over).items():
            assert n <= len(self.host[key]), (key, n)
            setattr(cols, field, self.dev[key])
        return cols

    def gpu(self, n, cutoff, f64_path=False, **over):
        cols = self.cols(n, **over)
        if f64_path:
            cols = without(cols, *INT_FIELDS)
        return self.sess.q1(cols, cutoff)

    def ref(self, n, cutoff, **over):
        """oracle result, computed once per distinct case"""
        key = (n, cutoff, tuple(sorted(over.items())))
        if key not in self._ref:
            cols = {f: self.host[k][:n] for f, k in self._names(over).items()
                    if f not in INT_FIELDS}
            self._ref[key] = oracle.q1_exact(cols, cutoff)[0]
        return self._ref[key]

    def check(self, n, cutoff, **over):
        g = self.gpu(n, cutoff, **over)
        assert_q1_equal(g, self.ref(n, cutoff, **over))
        return g


@pytest.fixture(scope="module")
def pool(sess):
    p = _Pool(sess)
    yield p
    p.close()


@pytest.mark.parametrize("n", SIZES)
def test_loop_boundaries(pool, n):
    """0/1/2 pipelined iterations per lane, with and without a tail"""
    g = pool.check(n, CUT_HALF)
    if n >= 1024:
        assert all(g.count[c] > 0 for c in range(6))   # all six combos present


@pytest.mark.parametrize("cutoff", [CUT_NONE, CUT_ALL, CUT_HALF])
@pytest.mark.parametrize("n", [1025, FULL + R + 1])
def test_cutoffs(pool, n, cutoff):
    g = pool.check(n, cutoff)
    total = sum(g.count)
    if cutoff == CUT_NONE:
        assert total == 0 and all(w == 0 for w in g.raw)
    elif cutoff == CUT_ALL:
        assert total == n
    else:
        assert 0.4 * n < total < 0.6 * n


def test_single_combo(pool):
    n = FULL + R + 1
    g = pool.check(n, CUT_ALL, returnflag="rf_single", linestatus="ls_single")
    assert g.count[5] == n and sum(g.count) == n


def test_one_row_selected(pool):
    g = pool.check(FULL + R + 1, CUT_HALF, shipdate="shipdate_one")
    assert sum(g.count) == 1


def test_decode_domain(pool):
    """every extendedprice_cents of the TPC-H domain once: one mis-rounded
    decode changes an exact sum"""
    g = pool.check(DOMAIN_N, CUT_ALL, extendedprice_cents="cents_domain",
                   quantity_u8="qty_domain", discount_pct="dpct_domain",
                   tax_pct="tpct_domain")
    assert sum(g.count) == DOMAIN_N


@pytest.mark.parametrize("n", [2 * FULL, 2 * FULL + R - 1])
def test_carries(pool, n):
    """every lane holds 2R rows of addends near 2^62.7 spread over two combos,
    so the low 64 bits wrap inside a lane and again in the wave/block/grid merge"""
    g = pool.check(n, CUT_ALL, extendedprice_cents="cents_big",
                   returnflag="rf_two", linestatus="ls_zero")
    for c in (0, 2):
        assert g.count[c] > 0
        assert g.raw[c * 10 + 1] != 0, ("sum_base high word", c)
        assert g.raw[c * 10 + 3] != 0 and g.raw[c * 10 + 5] != 0


def test_wide_bytes(pool):
    """quantity up to 255, discount_pct 99 and 100: the whole byte decodes like
    the f64 path"""
    over = dict(quantity_u8="qty_wide", discount_pct="dpct_wide")
    gi = pool.check(1025, CUT_ALL, **over)
    gf = pool.gpu(1025, CUT_ALL, f64_path=True, **over)
    assert list(gi.raw) == list(gf.raw)


def test_repeated_calls_one_session(pool):
    """integer path, f64 path, another n and cutoff, then the first again:
    nothing carries over from one call's result or partials to the next"""
    cases = [
        (2 * FULL + R - 1, CUT_ALL, False, dict(extendedprice_cents="cents_big")),
        (2 * FULL + R - 1, CUT_ALL, True, dict(extendedprice_cents="cents_big")),
        (1025, CUT_HALF, False, dict()),
        (FULL + 1, CUT_NONE, True, dict()),
        (2 * FULL + R - 1, CUT_ALL, False, dict(extendedprice_cents="cents_big")),
    ]
    got = [pool.gpu(n, cut, f64_path=f, **over) for n, cut, f, over in cases]
    for g, (n, cut, f, over) in zip(got, cases):
        assert_q1_equal(g, pool.ref(n, cut, **over))
    assert list(got[0].raw) == list(got[1].raw) == list(got[4].raw)
