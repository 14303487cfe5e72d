"""Fused Q1 kernel matrix: loop boundaries, combos, conversion domain, carries.

Hand-built columns are uploaded the way bench.py's parquet leg does
(tpch_queries._device_buffer + tg_copy_htod + a LineitemCols filled by hand)
and `sess.q1` is compared with `oracle.q1_exact` on the same numpy arrays.
The fused sums are error-free fixed-point, so every comparison is exact
equality — no tolerance anywhere in this file.

One pool of POOL_N rows per column variant is uploaded once; a case of n rows
runs on the first n rows of its columns (row_count = n), and the oracle on the
same prefix of the host arrays.
"""
import ctypes

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

# tg_q1_run caps the scan grid at GRID_CAP blocks of 256 lanes, 4 rows per lane
# per iteration, so a lane runs a second (pipelined) iteration only once
# n > FULL_ITER. The boundary sizes below are derived from that cap.
GRID_CAP = 1536
FULL_ITER = GRID_CAP * 256 * 4           # 1,572,864
POOL_N = 2 * FULL_ITER + 3               # 3,145,731
CUT_HALF = 10000                         # shipdate is uniform in [8000, 12000)
CUT_NONE = 0
CUT_ALL = 1 << 30

SIZES_TINY = [0, 1, 3, 4, 5, 255, 1024, 1025]
SIZES_ONE_TWO = [FULL_ITER - 1, FULL_ITER, FULL_ITER + 1, FULL_ITER + 4, FULL_ITER + 5]
SIZES_TWO = [2 * FULL_ITER, 2 * FULL_ITER + 1, 2 * FULL_ITER + 3]


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


def _host_pool():
    """Column variants, POOL_N rows each (seeded)."""
    rng = np.random.default_rng(20260)
    n = POOL_N
    h = {}
    h["shipdate"] = rng.integers(8000, 12000, n, dtype=np.int32)
    # all six combos in random order, A|O and R|O included
    h["returnflag"] = rng.integers(0, 3, n, dtype=np.uint8)
    h["linestatus"] = rng.integers(0, 2, n, dtype=np.uint8)
    h["quantity"] = rng.integers(1, 51, n).astype(np.float64)
    # discount: 0.0, 0.01..0.10 and values just below 1
    disc_set = np.array([0.0] + [i / 100.0 for i in range(1, 11)]
                        + [0.999, 1.0 - 2.0 ** -20, np.nextafter(1.0, 0.0)])
    h["discount"] = disc_set[rng.integers(0, len(disc_set), n)]
    h["tax"] = rng.integers(0, 9, n).astype(np.float64) / 100.0
    # prices: exact small values below 2^9, full-mantissa values in
    # [2^9, 2^17), and values up to 900,000.0 (charge * 2^43 < 2^63 at tax 0.08)
    small = np.array([100.25, 0.5, 1.0, 37.125, 511.75, 0.25])
    price = np.where(rng.random(n) < 0.5,
                     rng.uniform(512.0, 131072.0, n),
                     rng.uniform(131072.0, 900000.0, n))
    pick = rng.random(n)
    price = np.where(pick < 0.15, small[rng.integers(0, len(small), n)], price)
    price = np.where(pick > 0.99, 900000.0, price)
    h["extendedprice"] = price
    # variants
    h["rf_single"] = np.full(n, 2, np.uint8)        # every row R|O
    h["ls_single"] = np.full(n, 1, np.uint8)
    one = np.full(n, 11999, np.int32)               # one lane-row selected
    one[1_234_567] = 9000
    h["shipdate_one"] = one
    h["quantity_big"] = rng.integers(1, 1 << 38, n).astype(np.float64)
    # addends near 2^62.7: three same-combo rows wrap a lane's low word
    h["price_big"] = rng.uniform(880000.0, 900000.0, n)
    h["rf_two"] = rng.integers(0, 2, n, dtype=np.uint8)   # combos A|F, N|F only
    h["ls_zero"] = np.zeros(n, np.uint8)
    return h


class _Pool:
    def __init__(self, sess):
        import trino_amd
        from trino_amd import tpch_queries as tq
        self.sess, self.tq, self.trino_amd = sess, tq, trino_amd
        self.host = _host_pool()
        self.dev = {}
        for k, a in self.host.items():
            a = np.ascontiguousarray(a)
            self.host[k] = a
            p = tq._device_buffer(sess, a.nbytes)
            trino_amd._check(trino_amd._lib.tg_copy_htod(sess._h, p, a.ctypes.data, a.nbytes))
            self.dev[k] = p
        self._ref = {}

    def close(self):
        for p in self.dev.values():
            self.tq._device_free(self.sess, p)

    def _names(self, over):
        names = dict(shipdate="shipdate", quantity="quantity", extendedprice="extendedprice",
                     discount="discount", tax="tax", returnflag="returnflag",
                     linestatus="linestatus")
        names.update(over)
        return names

    def gpu(self, n, cutoff, **over):
        cols = self.trino_amd.LineitemCols()
        cols.row_count = n
        for field, key in self._names(over).items():
            setattr(cols, field, self.dev[key])
        return self.sess.q1(cols, cutoff)

    def ref(self, n, cutoff, **over):
        """oracle result, computed once per distinct case"""
        key = (n, cutoff, tuple(sorted(over.items())))
        if key not in self._ref:
            cols = {f: self.host[k][:n] for f, k in self._names(over).items()}
            self._ref[key] = oracle.q1_exact(cols, cutoff)[0]
        return self._ref[key]

    def check(self, n, cutoff, **over):
        g = self.gpu(n, cutoff, **over)
        assert_q1_equal(g, self.ref(n, cutoff, **over))
        return g


@pytest.fixture(scope="module")
def pool():
    import trino_amd
    s = trino_amd.Session(0)
    p = _Pool(s)
    yield p
    p.close()
    s.close()


@pytest.mark.parametrize("n", SIZES_TINY + SIZES_ONE_TWO + SIZES_TWO)
def test_loop_boundaries(pool, n):
    """0/1/2 pipelined iterations per lane, with and without a tail"""
    g = pool.check(n, CUT_HALF)
    if n >= 1024:
        assert all(g.count[c] > 0 for c in range(6))   # all six combos present


@pytest.mark.parametrize("cutoff", [CUT_NONE, CUT_ALL, CUT_HALF])
@pytest.mark.parametrize("n", [1025, FULL_ITER + 5])
def test_cutoffs(pool, n, cutoff):
    g = pool.check(n, cutoff)
    total = sum(g.count)
    if cutoff == CUT_NONE:
        assert total == 0 and all(w == 0 for w in g.raw)
    elif cutoff == CUT_ALL:
        assert total == n
    else:
        assert 0.4 * n < total < 0.6 * n


@pytest.mark.parametrize("n", [1025, FULL_ITER + 5])
def test_single_combo(pool, n):
    g = pool.check(n, CUT_ALL, returnflag="rf_single", linestatus="ls_single")
    assert g.count[5] == n and sum(g.count) == n


def test_one_row_selected(pool):
    n = FULL_ITER + 5
    g = pool.check(n, CUT_HALF, shipdate="shipdate_one")
    assert sum(g.count) == 1


@pytest.mark.parametrize("n", [1025, 2 * FULL_ITER + 3])
def test_large_quantities(pool, n):
    pool.check(n, CUT_ALL, quantity="quantity_big")


@pytest.mark.parametrize("n", [2 * FULL_ITER, 2 * FULL_ITER + 3])
def test_carry_out_of_low_word(pool, n):
    """every lane holds 8 rows of addends near 2^62.7 spread over two combos,
    so the low word wraps inside a lane and again in the wave/block/grid merge"""
    g = pool.check(n, CUT_ALL, extendedprice="price_big",
                   returnflag="rf_two", linestatus="ls_zero")
    for c in (0, 2):
        assert g.count[c] > 0
        assert g.raw[c * 10 + 1] != 0, ("sum_base high word", c)
        assert g.raw[c * 10 + 3] != 0 and g.raw[c * 10 + 5] != 0


def test_repeated_calls_one_session(pool):
    """three different inputs and cutoffs back to back, then the first again:
    nothing carries over from one call's result or partials to the next"""
    cases = [
        (2 * FULL_ITER + 3, CUT_ALL, dict(extendedprice="price_big")),
        (1025, CUT_HALF, dict()),
        (FULL_ITER + 1, CUT_NONE, dict(quantity="quantity_big")),
        (2 * FULL_ITER + 3, CUT_ALL, dict(extendedprice="price_big")),
    ]
    got = [pool.gpu(n, cut, **over) for n, cut, over in cases]
    for g, (n, cut, over) in zip(got, cases):
        assert_q1_equal(g, pool.ref(n, cut, **over))
    assert list(got[0].raw) == list(got[3].raw)
