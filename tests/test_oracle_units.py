"""Oracle unit pins: hashes, group-by contract, join chain order, partition.

Golden sources: public xxHash64 test vectors; the reference's constants
(AbstractLongType.java:121-125, CombineHashFunction.java:29-32,
BigintGroupByHash.java:297-300, GroupByHash.java:121-128 row-order contract,
ArrayPositionLinks.java:24-45 chain semantics, HashGenerator.java:41-46 and
LocalPartitionGenerator.java:76-80 partition reduction). Python reimplements
each formula independently to cross-check the C restatement.
"""
import math

import numpy as np
import pytest

import oracle

M64 = (1 << 64) - 1


def rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def py_bigint_hash(v):
    return (rotl((v & M64) * 0xC2B2AE3D27D4EB4F & M64, 31) * 0x9E3779B185EBCA87) & M64


def py_murmur3(h):
    h &= M64
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 33
    return h


def test_bigint_hash():
    for v in [0, 1, -1, 42, 2**62, -2**62, 123456789123456789]:
        assert oracle.bigint_hash(v) == py_bigint_hash(v)


def test_murmur3_mix():
    for v in [0, 1, 0xDEADBEEF, 2**63, M64]:
        assert oracle.murmur3_mix(v) == py_murmur3(v)


def test_combine_hash():
    assert oracle.combine_hash(0, 5) == 5
    assert oracle.combine_hash(7, 3) == 31 * 7 + 3
    # overflow wraps like Java long
    assert oracle.combine_hash(2**62, 2**62) == ((31 * 2**62 + 2**62 + 2**63) % 2**64) - 2**63


def test_double_hash_normalizes_negative_zero():
    assert oracle.double_hash(-0.0) == oracle.double_hash(0.0)
    assert oracle.double_hash(1.5) == py_bigint_hash(np.float64(1.5).view(np.int64).item())


def test_xxhash64_public_vectors():
    # public xxHash64 reference vectors, seed 0
    assert oracle.xxhash64(b"") == 0xEF46DB3751D8E999
    assert oracle.xxhash64(b"a") == 0xD24EC4F1A98C6E5B
    assert oracle.xxhash64(b"abc") == 0x44BC2CF5AD770999
    assert oracle.xxhash64(b"as") == 0x1C330FB2D66BE179
    assert oracle.xxhash64(b"asd") == 0x631C37CE72A97393
    assert oracle.xxhash64(b"asdf") == 0x415872F599CEA71E
    # >32 bytes path
    data = bytes(range(64))
    assert oracle.xxhash64(data) == oracle.xxhash64(data)  # deterministic
    # long-value specialization == bytes of LE long
    for v in [0, 1, -1, 123456789]:
        assert oracle.xxhash64_long(v) == oracle.xxhash64(
            int(v).to_bytes(8, "little", signed=True))


def test_partition_functions():
    for h in [0, 1, -5, 2**40, -2**40]:
        # local: (int)XxHash64.hash(Long.reverse(h)) & mask
        rev = int(bin(h & M64)[2:].zfill(64)[::-1], 2)
        x = oracle.xxhash64_long(rev - 2**64 if rev >= 2**63 else rev)
        assert oracle.partition_local(h, 8) == (x & 0xFFFFFFFF) % 2**32 & 7
        # remote: (unsigned(Long.hashCode(h)) * n) >>> 32
        lh = ((h & M64) ^ ((h & M64) >> 32)) & 0xFFFFFFFF
        assert oracle.partition_remote(h, 13) == (lh * 13) >> 32


def test_hash_rows_combine():
    k1 = np.array([1, 2, 3], np.int64)
    k2 = np.array([4.0, -0.0, 1.5], np.float64)
    h = oracle.hash_rows([k1, k2], [oracle.TG_BIGINT, oracle.TG_DOUBLE])
    for i in range(3):
        exp = (31 * py_bigint_hash(int(k1[i])) +
               py_bigint_hash(np.float64(abs(k2[i]) if k2[i] == 0 else k2[i]).view(np.int64).item())) & M64
        assert h[i] == exp


class TestBigintGroupBy:
    """Contract of GroupByHash.getGroupIds (GroupByHash.java:121-128):
    ids assigned in row order of first occurrence; null gets its own id."""

    def test_row_order_ids(self):
        keys = np.array([9, 9, 3, 9, 5, 3, 7], np.int64)
        gids, ng, vals, nullg = oracle.bigint_groupby(keys)
        assert list(gids) == [0, 0, 1, 0, 2, 1, 3]
        assert ng == 4 and list(vals) == [9, 3, 5, 7] and nullg == -1

    def test_null_group(self):
        keys = np.array([9, 0, 3, 0], np.int64)
        valid = np.array([0b0101], np.uint64)  # rows 1,3 null
        gids, ng, vals, nullg = oracle.bigint_groupby(keys, valid)
        assert list(gids) == [0, 1, 2, 1]
        assert ng == 3 and nullg == 1

    def test_rehash_preserves_ids(self):
        n = 100_000
        rng = np.random.default_rng(0)
        keys = rng.integers(0, 5000, n).astype(np.int64)
        gids, ng, vals, _ = oracle.bigint_groupby(keys)
        # ids must match first-occurrence order
        seen = {}
        exp = np.empty(n, np.int32)
        for i, k in enumerate(keys.tolist()):
            exp[i] = seen.setdefault(k, len(seen))
        assert np.array_equal(gids, exp) and ng == len(seen)
        assert np.array_equal(vals, np.array(list(seen.keys()), np.int64))


class TestFlatGroupBy:
    def test_multi_channel(self):
        c1 = np.array([1, 1, 2, 1, 2], np.int64)
        c2 = np.array([1.0, 2.0, 1.0, 1.0, 1.0], np.float64)
        gids, ng, first = oracle.flat_groupby([c1, c2], [oracle.TG_BIGINT, oracle.TG_DOUBLE])
        assert list(gids) == [0, 1, 2, 0, 2] and ng == 3
        assert list(first) == [0, 1, 2]

    def test_many_groups_rehash(self):
        n = 50_000
        rng = np.random.default_rng(1)
        c1 = rng.integers(0, 300, n).astype(np.int8)
        c2 = rng.integers(0, 50, n).astype(np.int32)
        gids, ng, first = oracle.flat_groupby([c1, c2], [oracle.TG_TINYINT, oracle.TG_INTEGER])
        seen = {}
        exp = np.empty(n, np.int32)
        for i in range(n):
            exp[i] = seen.setdefault((int(c1[i]), int(c2[i])), len(seen))
        assert np.array_equal(gids, exp) and ng == len(seen)


class TestJoin:
    def test_chain_order_reverse_insertion(self):
        """ArrayPositionLinks: duplicate key matches emit newest build row
        first, then links to older rows (DefaultPagesHash.insertValue)."""
        bk = np.array([10, 20, 10, 30, 10], np.int64)
        t = oracle.JoinTable(bk)
        op, ob = t.probe(np.array([10, 25, 30], np.int64))
        assert list(zip(op.tolist(), ob.tolist())) == [(0, 4), (0, 2), (0, 0), (2, 3)]

    def test_null_keys_never_match(self):
        bk = np.array([10, 20], np.int64)
        bvalid = np.array([0b01], np.uint64)  # row1 (20) is null
        t = oracle.JoinTable(bk, valid=bvalid)
        pk = np.array([20, 10], np.int64)
        pvalid = np.array([0b01], np.uint64)  # probe row1 (10) null
        op, ob = t.probe(pk, probe_valid=pvalid)
        assert len(op) == 0

    def test_load_factor_sizing(self):
        # IncrementalLoadFactorHashArraySizeSupplier: <=65536 -> 0.25
        t = oracle.JoinTable(np.arange(100, dtype=np.int64))
        assert t.table_size() == 512  # 100/0.25=400 -> 512

    def test_grouped_aggregation(self):
        gids = np.array([0, 1, 0, 1, 0], np.int32)
        vals = np.array([1.5, 2.0, 2.5, 3.0, -1.0], np.float64)
        s = oracle.grouped_sum_f64(gids, vals, 2)
        assert s[0] == 1.5 + 2.5 + -1.0 and s[1] == 5.0
        c = oracle.grouped_count(gids, 2)
        assert list(c) == [3, 2]


class TestAggregationMatrixHost:
    """Host-side checks for tests/test_gpu_aggregation_matrix.py: the key
    shape constructors reach the k_agg_update path their docstrings name
    (CPU simulation of the per-wave choice), the streaming shapes have the
    run ends they claim, and the module's reference matches hand-computed
    answers. No GPU, no oracle."""

    @staticmethod
    def mx():
        import test_gpu_aggregation_matrix as m
        return m

    @pytest.mark.parametrize("shape", ["uniform", "hot2", "hot8", "hot_then_tail",
                                       "bail", "interleaved", "scatter", "single"])
    def test_shape_reaches_named_path(self, shape):
        m = self.mx()
        assert set(m.SHAPES) == set(m.SHAPE_PATHS)
        assert m.SHAPES[shape].__doc__
        for n in m.SMALL_NS + (64 * 7,):
            g = m.SHAPES[shape](n)
            assert len(g) == n
            # distinct group indexes map to distinct keys
            assert len(set(m.key_of(g).tolist())) == len(set(g.tolist()))
            full = n // 64
            for s in range(full):
                assert m.simulate_wave(g[s * 64:(s + 1) * 64]) == m.SHAPE_PATHS[shape]
            if n % 64:     # partial last wave never takes the uniform path
                assert m.simulate_wave(g[full * 64:])["path"] == "hot"
        g = m.SHAPES[shape](1000)
        if shape == "uniform":
            assert all(g[s * 64] != g[(s + 1) * 64] for s in range(14))
        if shape == "interleaved":
            assert g[0] == g[2] != g[1] == g[3]

    def test_simulation_counts(self):
        m = self.mx()
        # 9 clusters of 7 + one lane: small first cluster bails after round 1
        assert m.simulate_wave([i // 7 for i in range(64)]) == dict(
            path="hot", exit="bail", rounds=1, first=7, leftover=57)
        # 9 groups, first of 8 lanes: 8 rounds, the ninth group is left over
        g = [i // 8 for i in range(56)] + [7] * 4 + [8] * 4
        assert m.simulate_wave(g) == dict(path="hot", exit="rounds8", rounds=8,
                                          first=8, leftover=4)
        # 64 equal ids but only 63 active lanes: not uniform
        assert m.simulate_wave([3] * 63) == dict(path="hot", exit="drained",
                                                 rounds=1, first=63, leftover=0)

    def test_streaming_shapes(self):
        m = self.mx()

        def end_lanes(name, n=1000):
            g = m.runs_to_gids(m.STREAM_SHAPES[name], n)
            assert len(g) == n and np.all(np.diff(g) >= 0)
            ends = np.flatnonzero(np.diff(g)) % 64
            return g, set(ends.tolist())

        g, ends = end_lanes("runs1")
        assert len(set(g.tolist())) == 1000
        g, ends = end_lanes("runs63_64_65")
        assert np.bincount(g)[:3].tolist() == [63, 64, 65]
        g, ends = end_lanes("run200")
        assert 200 in np.bincount(g).tolist()
        g, ends = end_lanes("ends62_63_0")
        assert ends == {62, 63, 0}
        assert m.GRID_STRIDE_N == 524_288 + 64 * 3 + 5

    def test_value_patterns(self):
        m = self.mx()
        from fractions import Fraction
        gid = np.asarray(m.SHAPES["hot2"](1000), np.int64)
        iv, fv, ew, em = m.value_cols(gid, 1)
        for c in (iv, fv, ew, em):
            assert 0.2 < 1 - c.valid.mean() < 0.4          # ~30 % NULLs
            assert c.valid[m.first_rows(gid)].all()
        assert iv.values[iv.valid].min() < -2 ** 38 and iv.values[iv.valid].max() > 2 ** 38
        m.assert_exact_precondition(ew.values[ew.valid], m.SP_WIDE)
        m.assert_exact_precondition(em.values[em.valid], m.SP_MONEY)
        with pytest.raises(AssertionError):
            m.assert_exact_precondition(np.array([0.1]), 20)
        with pytest.raises(AssertionError):
            m.assert_exact_precondition(np.array([2.0 ** 44]), 20)
        sums = []
        for g in sorted(set(gid.tolist())):
            sel = (gid == g) & ew.valid
            sums.append(sum(Fraction(x) for x in ew.values[sel].tolist()))
        scaled = [s * 2 ** m.SP_WIDE for s in sums]
        assert any(abs(s) >= 2 ** 64 for s in scaled)        # crosses 2^64
        assert any(s > 0 for s in scaled) and any(s < 0 for s in scaled)
        assert any(Fraction(float(s)) != s for s in sums)    # > 53 bits: rounds

    def test_reference_tiny_ints_and_nulls(self):
        m = self.mx()
        k = m.Col(np.array([7, -2, 7, -2, 7, 9], np.int64))
        v = m.Col(np.array([5, 1, -8, m.POISON_I, 3, m.POISON_I], np.int64),
                  [1, 1, 1, 0, 1, 0])
        aggs = [m.Agg(m.COUNT_STAR), m.Agg(m.COUNT_COL, 1), m.Agg(m.SUM_I64, 1),
                m.Agg(m.MIN_I64, 1), m.Agg(m.MAX_I64, 1)]
        r = m.reference([k, v], [0], aggs)
        assert r.keys == [(7,), (-2,), (9,)]            # first-occurrence order
        assert r.cols == [[3, 2, 1], [3, 1, 0], [0, 1, None],
                          [-8, 1, None], [5, 1, None]]
        assert r.sizes == [3, 2, 1]
        with pytest.raises(AssertionError):
            m.assert_sums_defined(r, aggs)
        # wraparound: Python's sum reduced mod 2^64
        w = m.reference([m.Col(np.zeros(2, np.int64)),
                         m.Col(np.array([2 ** 62 + 5, 2 ** 62 + 7], np.int64))],
                        [0], [m.Agg(m.SUM_I64, 1)])
        assert w.cols == [[-2 ** 63 + 12]]

    def test_reference_tiny_mask_and_two_channel_key(self):
        m = self.mx()
        k1 = m.Col(np.array([1, 1, 1, 2, 2, 1], np.int64))
        k2 = m.Col(np.array([0, 5, 0, 5, 5, 0], np.int32), [1, 1, 1, 1, 1, 0])
        v = m.Col(np.array([10, 20, 30, 40, 50, 60], np.int64))
        a = m.Col(np.array([3, -1, 9, -4, -9, 9], np.int32), [1, 1, 0, 1, 1, 1])
        b = m.Col(np.array([-3, -2, 0, -4, -8, 8], np.int64))
        aggs = [m.Agg(m.COUNT_STAR, -1, 0, (3, 4)), m.Agg(m.SUM_I64, 2, 0, (3, 4)),
                m.Agg(m.MIN_I64, 2, 0, (3, 4)), m.Agg(m.MAX_I64, 2)]
        r = m.reference([k1, k2, v, a, b], [0, 1], aggs)
        # groups: (1,0) rows 0,2; (1,5) row 1; (2,5) rows 3,4; (1,NULL) row 5
        assert r.keys == [(1, 0), (1, 5), (2, 5), (1, None)]
        # gate a > b: row0 yes, row1 yes, row2 NULL a -> no, row3 -4 > -4 no,
        # row4 -9 > -8 no, row5 yes; group (2,5) is masked out entirely
        assert r.cols == [[1, 1, 0, 1], [10, 20, None, 60],
                          [10, 20, None, 60], [30, 20, 50, 60]]
        assert aggs[0].spec() == (m.COUNT_STAR, -1, 0, 3, 4)
        assert aggs[3].spec() == (m.MAX_I64, 2, 0)

    def test_reference_tiny_doubles(self):
        m = self.mx()
        from fractions import Fraction
        k = m.Col(np.array([4, 4, 4, 6, 6], np.int64))
        big = 2.0 ** 60
        v = m.Col(np.array([big, 1.0, -big, 0.5, np.nan]), [1, 1, 1, 1, 0])
        aggs = [m.Agg(m.SUM_F64_EXACT, 1, 1), m.Agg(m.SUM_F64, 1), m.Agg(m.AVG_F64, 1)]
        r = m.reference([k, v], [0], aggs)
        assert r.keys == [(4,), (6,)]
        assert r.cols[0] == [1.0, 0.5]          # exact: cancellation keeps the 1
        assert r.cols[0][0] == float(Fraction(big) + 1 - Fraction(big))
        assert r.cols[1] == [1.0, 0.5]
        assert r.cols[2] == [1.0 / 3.0, 0.5]
        # bounds: n_g * 2^-53 * sum|v|; AVG: that / count + 2^-53 * |avg|
        assert r.bounds[0] is None
        assert r.bounds[1] == [3 * 2.0 ** -53 * (2 * big + 1), 2 * 2.0 ** -53 * 0.5]
        assert r.bounds[2] == [r.bounds[1][0] / 3 + 2.0 ** -53 / 3.0,
                               r.bounds[1][1] / 1 + 2.0 ** -53 * 0.5]
        # scalar aggregation of nothing: one group, COUNT 0, AVG NULL
        e = m.reference([m.Col(np.zeros(0, np.int64)), m.Col(np.zeros(0))], [],
                        [m.Agg(m.COUNT_STAR), m.Agg(m.AVG_F64, 1)])
        assert e.keys == [()] and e.cols == [[0], [None]]

    def test_validity_packing_and_dense_reference(self):
        m = self.mx()
        v = np.arange(130) % 3 != 0
        w = m.pack_valid(v)
        assert len(w) == 3 and int(w[0]) & 0b111 == 0b110
        assert np.array_equal(m.unpack_valid(w, 130), v)
        assert m.unpack_valid(None, 5).all()
        k = m.Col(np.array([5, 2, 9, 2, 5, 2], np.int32), [1, 1, 1, 1, 0, 1])
        x = m.Col(np.array([4, 1, 7, -1, 8, m.POISON_I], np.int64), [1, 1, 1, 1, 1, 0])
        r = m.dense_reference([k, x], 2, 5, m.Agg(m.SUM_I64, 1))
        # key 9 out of range, row 4 NULL key; key 2 sums to 0 and is a group
        assert sorted(zip(r.keys, r.cols[0])) == [((2,), 0), ((5,), 4)]


class TestJoinMatrixHost:
    """Host-side checks for tests/test_gpu_join_matrix.py: its reference
    gives hand-computed answers, the vectorised twin and the oracle's
    independent join agree with it, every key shape constructor has the
    property its docstring claims, and every size constant equals the value
    derived from the constants parsed out of the sources. No GPU."""

    @staticmethod
    def mx():
        import test_gpu_join_matrix as m
        return m

    def test_ref_join_by_hand(self):
        m = self.mx()
        nan = float("nan")
        build = [(7,), (3,), (7,), (None,), (7,)]
        probe = [(7,), (4,), (None,), (3,)]
        # duplicates descending; NULL never matches; outer misses emit one row
        assert m.ref_join(build, probe, False) == [(0, 4), (0, 2), (0, 0), (3, 1)]
        assert m.ref_join(build, probe, True) == [
            (0, 4), (0, 2), (0, 0), (1, None), (2, None), (3, 1)]
        # a NULL in any component; integers by value
        assert m.ref_join([(1, None), (1, 2), (None, 2)], [(1, 2), (1, None)],
                          True) == [(0, 1), (1, None)]
        # NaN matches nothing, not even the same object; -0.0 matches 0.0
        assert m.ref_join([(nan,), (0.0,), (-0.0,)], [(nan,), (-0.0,), (0.0,)],
                          True) == [(0, None), (1, 2), (1, 1), (2, 2), (2, 1)]
        assert m.ref_join([(m.NAN_A,), (m.NAN_B,)], [(m.NAN_A,), (m.NAN_B,)],
                          False) == []
        # VARCHAR by bytes: '' is a value, not NULL
        assert m.ref_join([(b"",), (b"a",), (None,)], [(b"",), (None,), (b"a\0",)],
                          False) == [(0, 0)]
        assert m.ref_join([], [(1,), (None,)], False) == []
        assert m.ref_join([], [(1,), (None,)], True) == [(0, None), (1, None)]

    def test_ref_semi_by_hand(self):
        m = self.mx()
        nan = float("nan")
        assert m.ref_semi([(1,), (2,)], [(1,), (3,), (None,)]) == [True, False, None]
        # a miss against a build that contains a NULL key is NULL; a hit stays True
        assert m.ref_semi([(1,), (None,)], [(1,), (3,), (None,)]) == [True, None, None]
        # NULL IN (empty) is False
        assert m.ref_semi([], [(1,), (None,)]) == [False, False]
        assert m.ref_semi([(nan,), (0.0,)], [(nan,), (-0.0,)]) == [False, True]
        assert m.ref_semi([(nan,), (None,)], [(nan,)]) == [None]

    def test_vectorised_twin_equals_ref_join(self):
        m = self.mx()
        r = np.random.default_rng(1)
        for trial in range(40):
            nb, mm = int(r.integers(0, 40)), int(r.integers(0, 40))
            bk = r.integers(-4, 5, nb).astype(np.int64) * 2 ** 40
            pk = r.integers(-5, 6, mm).astype(np.int64) * 2 ** 40
            bv = r.random(nb) > 0.2 if trial % 3 else None
            pv = r.random(mm) > 0.2 if trial % 2 else None
            bkeys = [(int(k) if bv is None or bv[i] else None,) for i, k in enumerate(bk)]
            pkeys = [(int(k) if pv is None or pv[i] else None,) for i, k in enumerate(pk)]
            op, ob = m.ref_join_vec(bk, bv, pk, pv)
            assert list(zip(op.tolist(), ob.tolist())) == m.ref_join(bkeys, pkeys, False)
            hit, null = m.ref_semi_vec(bk, bv, pk, pv)
            got = [None if z else bool(h) for h, z in zip(hit, null)]
            assert got == m.ref_semi(bkeys, pkeys)

    def test_ref_join_equals_oracle_join(self):
        """two independent implementations, single BIGINT keys"""
        m = self.mx()
        for shape in ("unique", "dups", "nulls", "colliding", "one_hot"):
            nb = 1000
            bk, bnull, pk, pnull = m.SHAPES[shape](nb, 300, seed=3)
            bvalid = None if bnull is None else m.pack_bits(~bnull)
            pvalid = None if pnull is None else m.pack_bits(~pnull)
            t = oracle.JoinTable(bk, valid=bvalid)
            op, ob = t.probe(pk, probe_valid=pvalid, cap=10 ** 6)
            build, probe = m.bigint_tables(bk, bnull, pk, pnull)
            ref = m.ref_join(m.keys_of(build, [0]), m.keys_of(probe, [0]), False)
            assert sorted(zip(op.tolist(), ob.tolist())) == sorted(ref)

    def test_size_constants_follow_the_sources(self):
        m = self.mx()
        c = m.source_constants()
        assert m.JREG_SLOTS == c["JREG_SLOTS"] and m.JSCAN_CHUNK == c["JSCAN_CHUNK"]
        assert m.WAVE == 64
        assert m.GRID_THREADS == c["TG_BLOCK"] * c["TG_MAX_BLOCKS"]
        assert m.GRID_STRIDE_M > m.GRID_THREADS and m.GRID_STRIDE_M % 64 not in (0, 63)
        (l1, f1), (l2, f2), (_, f3) = c["LOAD"]
        assert (f1, f2, f3) == (0.25, 0.5, 0.75)
        # region edge: the last build size with one region, the first with two
        lo, hi = m.REGION_BUILDS
        assert hi == lo + 1
        assert m.join_hash_size(lo) == c["JREG_SLOTS"]
        assert m.join_hash_size(hi) == 2 * c["JREG_SLOTS"]
        # load-factor step
        assert m.LOAD_BUILDS == (l1, l1 + 1)
        assert m.join_hash_size(l1) == l1 * 4 and m.join_hash_size(l1 + 1) == l1 * 4
        assert m.join_hash_size(l1 + 1) < (l1 + 1) * 4     # now half full at most
        # the big build: second load-factor step, 64 regions, a second stride
        # in every build kernel, and a table that is cut into two partitions
        assert m.BIG_BUILD == l2 and m.join_hash_size(l2) == 2 * l2
        assert m.join_hash_size(l2) // c["JREG_SLOTS"] == 64
        assert m.BIG_BUILD > m.GRID_THREADS
        tbl = m.join_hash_size(l2) * 4 + l2 * 12
        assert c["PART_BYTES"] < tbl <= 2 * c["PART_BYTES"]
        # probe page edges around the scan chunk: one, two and three chunks
        ch = c["JSCAN_CHUNK"]
        assert set(m.PROBE_EDGES) >= {1, 63, 64, 65, ch - 1, ch, ch + 1, 2 * ch + 1}
        assert m.join_hash_size(0) == 2 and m.join_hash_size(1) == 4
        for nb in m.SMALL_BUILDS:
            assert m.join_hash_size(nb) <= c["JREG_SLOTS"]
        # murmur3 restatement against this file's independent Python one
        ks = np.array([0, 1, -1, 2 ** 40, -2 ** 40], np.int64)
        assert m.murmur3_mix(ks.view(np.uint64)).tolist() == [
            py_murmur3(int(k)) for k in ks]

    def test_key_shapes(self):
        m = self.mx()
        for shape, fn in m.SHAPES.items():
            assert fn.__doc__
            for nb in m.SMALL_BUILDS + (8193,):
                if nb < m.MIN_BUILD.get(shape, 0):
                    continue
                bk, bnull, pk, pnull = fn(nb, m.SMALL_M, seed=nb)
                assert len(bk) == nb and len(pk) == m.SMALL_M
                assert bk.dtype == np.int64 and pk.dtype == np.int64
                assert bnull is None or len(bnull) == nb
                assert pnull is None or len(pnull) == m.SMALL_M
        bk, _, pk, _ = m.shape_unique(1000, 400)
        assert len(set(bk.tolist())) == 1000
        assert (np.abs(bk) > 2 ** 31).mean() > 0.99 and (bk < 0).any() and (bk > 0).any()
        hits = np.isin(pk, bk)
        assert hits[0::2].all() and not hits[1::2].any()
        bk, _, pk, _ = m.shape_dups(1000, 400)
        copies = np.unique(bk, return_counts=True)[1]
        assert set(copies.tolist()) == {1, 2, 3, 4}
        assert np.any(np.diff(bk) < 0)                       # shuffled
        assert np.isin(pk, bk).mean() == 0.5
        bk, _, pk, _ = m.shape_one_hot(1000, 400)
        vals, copies = np.unique(bk, return_counts=True)
        assert copies.max() == m.ONE_HOT_COPIES == 500 and (copies == 1).sum() == 500
        assert (pk == vals[np.argmax(copies)]).sum() >= 100
        bk, _, pk, _ = m.shape_all_miss(1000, 400)
        assert not np.isin(pk, bk).any()
        bk, _, pk, pnull = m.shape_all_null_probe(1000, 400)
        assert pnull.all() and np.isin(pk, bk).all()         # would match if read
        bk, bnull, pk, pnull = m.shape_nulls(1000, 400)
        assert 0.01 < bnull.mean() < 0.06 and 0.01 < pnull.mean() < 0.06
        assert np.isin(bk[bnull], pk).any()                  # would match if read
        assert np.isin(pk[pnull], bk).any()
        # a key held by a NULL build row only is asked for by a valid probe row
        bk, bnull, pk, pnull = m.shape_nulls(1, 5)
        assert bnull.all() and (pk[~pnull] == bk[0]).any()

    @pytest.mark.parametrize("nb", [6, 63, 64, 65, 1000, 8193])
    def test_colliding_shape(self, nb):
        m = self.mx()
        cap = m.join_hash_size(nb)
        bk, _, pk, _ = m.shape_colliding(nb, m.SMALL_M)
        bslot = m.slots_of(bk, cap)
        a, d, b, e, c = (int(k) for k in pk[:5])
        slot = int(m.slots_of(np.array([a]), cap)[0])
        # the slot of A holds exactly the three distinct keys A, B and C
        in_slot = bk[bslot == slot]
        assert sorted(set(in_slot.tolist())) == sorted([a, b, c]) and len({a, b, c}) == 3
        assert sorted(np.unique(in_slot, return_counts=True)[1].tolist()) == [1, 2, 3]
        # D lands there and is absent; E lands in a slot no build key uses
        assert int(m.slots_of(np.array([d]), cap)[0]) == slot and d not in bk
        assert int(m.slots_of(np.array([e]), cap)[0]) not in set(bslot.tolist())
        assert len(set(bk.tolist())) == nb - 3
        # python restatement of the slot function agrees with numpy's
        assert py_murmur3(a) & (cap - 1) == slot

    def test_overflow_case_exceeds_first_cap(self):
        m = self.mx()
        bk, _, pk, _ = m.overflow_inputs()
        n = m.OVERFLOW_N
        assert len(bk) == len(pk) == n and len(set(bk.tolist()) | set(pk.tolist())) == 1
        midx = len(pk)                        # non-NULL probe rows
        src = open(m.os.path.join(m._CSRC, "ops_join.hip")).read()
        assert "int64_t cap = midx + t.n + 64;" in src
        assert n * n > midx + len(bk) + 64

    def test_set_and_page_shapes(self):
        m = self.mx()
        s = m.set_shapes()
        assert set(s) == set(m.SET_SHAPES)
        rng_of = lambda k: int(k.max()) - int(k.min()) + 1
        assert rng_of(s["range64"][0]) == 64 and rng_of(s["range65"][0]) == 65
        assert rng_of(s["range128"][0]) == 128
        assert s["runs_cross_words"][0].min() < 0
        k = s["clustered"][0]
        assert np.all(np.diff(k) >= 0)
        # many lanes of a wave share a word: 64 sorted neighbours span few words
        w = (k - k.min()) >> 6
        assert max(len(set(w[i:i + 64].tolist())) for i in range(0, len(k), 64)) <= 3
        assert len(s["n_not_multiple_of_64"][0]) % 64 and len(k) % 64
        k, z = s["nulls_inside_run"]
        assert z is not None and any(z[i] and k[i - 1] == k[i] == k[i + 1] and
                                     not z[i - 1] and not z[i + 1]
                                     for i in range(1, len(k) - 1))
        k = s["runs_cross_words"][0]
        w = (k - k.min()) >> 6
        assert np.any((np.diff(w) == 1) & (np.diff(k) <= 1))   # a run crosses a word
        assert max(m.WIDE_RANGE_KEYS) - min(m.WIDE_RANGE_KEYS) + 1 > 2 ** 33
        # multi-page build: NULL rows only in pages that carry a bitmap, at odd
        # bit offsets, first and last row of such a page included
        assert m.MULTI_PAGE_SIZES == [37, 64, 0, 1, 100, 8000]
        starts = np.cumsum([0] + m.MULTI_PAGE_SIZES)
        assert any(st % 64 for st in starts[1:-1])
        for shift in (1, 2):
            for mask in m._multi_page_masks(shift):
                assert mask.any()
                for i, bm in enumerate(m.MULTI_PAGE_BITMAPS):
                    if not bm:
                        assert not mask[starts[i]:starts[i + 1]].any()
        knull = m._multi_page_masks(1)[0]
        assert knull[37] and knull[100] and knull[102] and knull[-1]
        assert 0 < sum(m.MULTI_PAGE_BITMAPS) < len(m.MULTI_PAGE_BITMAPS)

    def test_generic_tables_and_packing(self):
        m = self.mx()
        for name in m.GENERIC:
            build, bk, probe, pk = m.generic_tables(name)
            assert [c.kind for c in build] == [c.kind for c in probe]
            bkeys, pkeys = m.keys_of(build, bk), m.keys_of(probe, pk)
            ref = m.ref_join(bkeys, pkeys, True)
            matched = [p for p in ref if p[1] is not None]
            assert matched and len(matched) < len(ref)         # hits and misses
            assert len(matched) > len({p for p, _ in matched})  # duplicates
        build, bk, probe, pk = m.generic_tables("bigint_integer")
        keys = m.keys_of(build, bk)
        assert any(k[0] is None and k[1] is not None for k in keys)
        assert any(k[1] is None and k[0] is not None for k in keys)
        build, bk, probe, pk = m.generic_tables("varchar_bigint")
        assert any(k[0] == b"" for k in m.keys_of(build, bk))   # '' is a value
        assert any(k[0] is None for k in m.keys_of(build, bk))
        build, bk, probe, pk = m.generic_tables("smallint_tinyint_date")
        assert all(min(k[i] for k in m.keys_of(build, bk)) < 0 for i in range(3))
        build, bk, probe, pk = m.generic_tables("double")
        bits = set(build[0].values.view(np.uint64).tolist())
        assert {0x7FF8000000000000, 0xFFF8000000000ABC, 0x8000000000000000, 0} <= bits
        v = np.arange(130) % 3 != 0
        w = m.pack_bits(v)
        assert len(w) == 3 and int(w[0]) & 0b111 == 0b110
        assert np.array_equal(m.unpack_bits(w, 130), v)
        assert m.unpack_bits(None, 5).all()
        for src_nulls in (False, True):
            build, probe = m.outer_column_tables(src_nulls)
            assert [c.kind for c in build] == ["i64", "i64", "f64", "i32", "date",
                                               "i16", "i8", "str", "i64"]
            assert all((c.valid is not None) == src_nulls for c in build[1:-1])


class TestFilterMatrixHost:
    """Host-side checks for tests/test_gpu_filter_matrix.py: ref_eval gives
    hand-computed answers, the size constants equal the ones parsed from the
    sources, and every program that claims a path takes it by construction.
    No GPU."""

    @staticmethod
    def mx():
        import test_gpu_filter_matrix as m
        return m

    def test_constants_match_sources(self):
        m = self.mx()
        k = m.source_constants()
        assert (k["CHUNK"], k["FSCAN_CHUNK"], k["FTERM_MAX"], k["MAX_STACK"]) == \
            (m.CHUNK, m.FSCAN_CHUNK, m.FTERM_MAX, m.MAX_STACK)
        assert k["TG_BLOCK"] * k["TG_MAX_BLOCKS"] == m.GRID_THREADS
        assert m.GRID_N == m.GRID_THREADS + 257
        assert k["SCAN_SMALL_FACTOR"] == 2
        small = k["SCAN_SMALL_FACTOR"] * k["FSCAN_CHUNK"]
        assert m.VARCHAR_COUNTS == (0, 1, small, small + 1, small + k["FSCAN_CHUNK"] + 1)
        assert max(m.EDGE_SIZES) // m.CHUNK + 1 <= small     # chunk scans stay one launch
        assert m.EDGE_SIZES == (0, 1, 63, 64, 65, m.CHUNK - 1, m.CHUNK, m.CHUNK + 1,
                                2 * m.CHUNK + 7)
        sizes = m.edge_sizes()
        assert len(set(sizes)) == len(sizes)
        for n in m.EDGE_SIZES:
            assert n in sizes
            assert n < 63 or any(s % 8 and 0 <= s - n <= 3 for s in sizes)

    def test_kleene_truth_tables(self):
        m = self.mx()
        T, Fa, N = 1, 0, None
        C, ev = m.C, m.ref_eval

        def tri(prog, row):
            v = ev(prog, row)
            return None if v[2] else bool(v[0])

        and_ = {(T, T): True, (T, Fa): False, (Fa, T): False, (Fa, Fa): False,
                (T, N): None, (N, T): None, (Fa, N): False, (N, Fa): False, (N, N): None}
        or_ = {(T, T): True, (T, Fa): True, (Fa, T): True, (Fa, Fa): False,
               (T, N): True, (N, T): True, (Fa, N): None, (N, Fa): None, (N, N): None}
        for (a, b), want in and_.items():
            assert tri((C(0), C(1), "and"), (a, b)) is want, (a, b)
        for (a, b), want in or_.items():
            assert tri((C(0), C(1), "or"), (a, b)) is want, (a, b)
        assert [tri((C(0), "not"), (a,)) for a in (T, Fa, N)] == [False, True, None]
        # a filter keeps a row iff the result is non-NULL and truthy
        assert [m.ref_keep((C(0),), (a,)) for a in (T, Fa, N, 2.5, 0.0, -0.0)] == \
            [True, False, False, True, False, False]

    def test_division_and_coercion(self):
        m = self.mx()
        C, I, F, ev = m.C, m.I, m.F, m.ref_eval
        assert ev((C(0), C(1), "div"), (7, 2)) == (3, True, False)
        assert ev((C(0), C(1), "div"), (-7, 2)) == (-3, True, False)     # toward zero
        assert ev((C(0), C(1), "div"), (7, -2)) == (-3, True, False)
        assert ev((C(0), C(1), "div"), (7, 0))[2] is True                # int / 0 = NULL
        assert ev((C(0), C(1), "div"), (None, 0))[2] is True
        assert ev((C(0), C(1), "div"), (7.0, 0)) == (float("inf"), False, False)
        assert ev((C(0), C(1), "div"), (-7, 0.0)) == (float("-inf"), False, False)
        assert ev((C(0), C(1), "div"), (7.0, -0.0)) == (float("-inf"), False, False)
        v = ev((C(0), C(1), "div"), (0.0, 0))
        assert v[0] != v[0] and not v[2]
        # mixed int/double coerces with float(i): 2^53+1 rounds to 2^53
        big = 2 ** 53 + 1
        assert ev((C(0), F(float(2 ** 53)), "eq"), (big,)) == (1, True, False)
        assert ev((C(0), I(2 ** 53), "eq"), (big,)) == (0, True, False)  # exact lane
        assert ev((C(0), F(0.0), "add"), (big,)) == (float(2 ** 53), False, False)
        assert ev((C(0), I(1), "add"), (big,)) == (big + 1, True, False)
        with pytest.raises(m.LeftInt64):
            ev((C(0), C(0), "mul"), (2 ** 32,))

    def test_nan_compares_and_between(self):
        m = self.mx()
        C, ev = m.C, m.ref_eval
        nan = float("nan")
        for op in m.CMPS:
            want = 1 if op == "ne" else 0
            assert ev((C(0), C(1), op), (nan, 1.0)) == (want, True, False), op
            assert ev((C(0), C(1), op), (1, nan)) == (want, True, False), op
            assert ev((C(0), C(1), op), (nan, nan)) == (want, True, False), op
        assert ev((C(0), C(1), "eq"), (0.0, -0.0))[0] == 1

        def btw(a, lo, hi):
            v = ev((C(0), C(1), C(2), "between"), (a, lo, hi))
            return None if v[2] else bool(v[0])

        assert btw(5, 1, 9) is True and btw(5, 6, 9) is False and btw(5, 9, 1) is False
        assert btw(5, None, 9) is None and btw(5, 1, None) is None
        assert btw(5, None, 4) is False and btw(5, 6, None) is False     # false dominates
        assert btw(None, 1, 9) is None and btw(5, None, None) is None
        assert btw(5, 1, nan) is False and btw(nan, 1, 9) is False
        assert btw(2 ** 53 + 1, float(2 ** 53), 2 ** 53 + 1) is True

    def test_path_claims_hold_by_construction(self):
        m = self.mx()
        cap = m.source_constants()["FTERM_MAX"]
        wide = m.chain(*m.WIDE)
        assert len(m.WIDE) == cap + 1 and m.count_terms(wide) == cap + 1
        assert m.path_of(wide) == "flags"
        assert m.count_terms(m.chain(*m.WIDE[:cap])) == cap
        n_terms = n_miss = 0
        for prog, path in m.terms_programs():
            assert m.path_of(prog) == path, prog
            assert m.stack_profile(prog)[1:] == (1, False)
            if path == "terms":
                n_terms += 1
            elif prog != wide:
                n_miss += 1
                assert m.count_terms(prog) == 0, prog      # really breaks the grammar
        assert n_terms >= 20 and n_miss >= 5
        for prog in m.flags_programs():
            assert m.path_of(prog) == "flags", prog
            mx_, sp, under = m.stack_profile(prog)
            assert mx_ <= m.MAX_STACK and sp == 1 and not under
        assert max(m.stack_profile(p)[0] for p in m.flags_programs()) == m.MAX_STACK
        assert m.stack_profile(m.deep_program(m.MAX_STACK + 1))[0] == m.MAX_STACK + 1
        for name, prog in m.GRID_FILTERS:
            assert m.path_of(prog) == name
        for prog in m.EDGE_PROGS:
            assert m.ref_filter(prog, [(1,), (0,), (1,)]) == [0, 2]
        assert [m.path_of(p) for p in m.EDGE_PROGS] == ["cmp", "terms", "flags"]

    def test_random_programs_stay_in_int64_and_select(self):
        m = self.mx()
        assert len(m.RANDOM_SEEDS) == 64 == len(set(m.RANDOM_SEEDS))
        cols, rows = m.random_page()
        assert [c.kind for c in cols] == list(m.KINDS)
        assert all(c.valid is not None and not c.valid.all() for c in cols)
        for c in cols:
            assert np.abs(c.values).max() < 2 ** 31
        useful = 0
        for seed in m.RANDOM_SEEDS:
            prog, kept = m.random_reference(seed)          # raises LeftInt64 on overflow
            mx_, sp, under = m.stack_profile(prog)
            assert mx_ <= m.MAX_STACK and sp == 1 and not under, seed
            for it in prog:
                if isinstance(it, tuple) and it[0] != "col":
                    assert abs(it[1]) <= 2 ** 31
            useful += 0.05 <= len(kept) / len(rows) <= 0.95
        assert useful >= len(m.RANDOM_SEEDS) // 4, useful

    def test_patterns(self):
        m = self.mx()
        n = 2 * m.CHUNK + 7
        assert m.pattern_flags("lane63", n).sum() == n // 64
        last = np.flatnonzero(m.pattern_flags("chunk_last", n))
        assert last.tolist() == [m.CHUNK - 1, 2 * m.CHUNK - 1, n - 1]
        a, b = m.pattern_flags("first_chunk_only", n), m.pattern_flags("second_chunk_only", n)
        assert a[:m.CHUNK].all() and not a[m.CHUNK:].any()
        assert b[m.CHUNK:2 * m.CHUNK].all() and not b[:m.CHUNK].any() and not b[2 * m.CHUNK:].any()


class TestOrderingMatrixHost:
    """Host-side checks for tests/test_gpu_ordering_matrix.py: the TopN
    reference by hand, the page shapes against the parsed path threshold and
    the partitioner shape list. No GPU."""

    @staticmethod
    def mx():
        import test_gpu_ordering_matrix as m
        return m

    def test_ref_topn_by_hand(self):
        m = self.mx()
        nan, inf = float("nan"), float("inf")
        keys = [(1.0,), (None,), (nan,), (-0.0,), (0.0,), (-nan,), (inf,), (-inf,), (None,)]
        asc = [m.canon_key(keys[i]) for i in m.ref_topn(keys, [0], 99)]
        assert asc == [(-inf,), (0.0,), (0.0,), (1.0,), (inf,), ("nan",), ("nan",),
                       (None,), (None,)]
        desc = [m.canon_key(keys[i]) for i in m.ref_topn(keys, [1], 99)]
        assert desc == asc[::-1]
        assert m.ref_topn(keys, [0], 3)[0] == 7 and len(m.ref_topn(keys, [0], 3)) == 3
        # ties on the leading key are broken by the second, each in its direction
        keys = [(2, 1.0), (1, nan), (2, None), (1, 5.0), (None, 0.0), (2, -3.0)]
        assert m.ref_topn(keys, [0, 0], 6) == [3, 1, 5, 0, 2, 4]
        assert m.ref_topn(keys, [0, 1], 6) == [1, 3, 2, 0, 5, 4]
        assert m.ref_topn(keys, [1, 0], 6) == [4, 5, 0, 2, 3, 1]
        assert m.ref_topn(keys, [0, 0], 2) == [3, 1]
        # INT64 extremes stay apart from NULL
        big = [(2 ** 63 - 1,), (None,), (-2 ** 63,)]
        assert m.ref_topn(big, [0], 3) == [2, 0, 1] and m.ref_topn(big, [1], 3) == [1, 0, 2]
        assert m.canon_key((-0.0, None, -nan, 3)) == (0.0, None, "nan", 3)

    def test_topn_shapes_hit_the_threshold(self):
        m = self.mx()
        k = m.source_constants()
        assert k["TOPN_DEVICE_ROWS"] == m.TOPN_DEVICE_ROWS == m.PATH_ROWS["device"]
        assert m.PATH_ROWS["host"] == 1000 < k["TOPN_DEVICE_ROWS"]
        assert m.page_sizes(m.TOPN_DEVICE_ROWS) == (1, 0, k["TOPN_DEVICE_ROWS"] - 2, 1)
        assert sum(m.page_sizes(m.TOPN_DEVICE_ROWS)) == k["TOPN_DEVICE_ROWS"]
        assert sum(m.page_sizes(m.TOPN_DEVICE_ROWS - 1)) == k["TOPN_DEVICE_ROWS"] - 1
        assert sum(m.page_sizes(m.HOST_ROWS)) == 1000
        for name in ("int64_extremes", "double_specials", "all_ones_nan"):
            c = m.special_cols(name, 1000, 12)
            assert 100 < (~c.valid).sum() < 400
        bits = m.special_cols("all_ones_nan", 1000, 12).values.view(np.uint64)
        assert (bits == 0x7FFFFFFFFFFFFFFF).any()
        d = m.special_cols("double_specials", 1000, 12).values
        assert np.isnan(d).any() and (np.signbit(d) & np.isnan(d)).any()
        assert (np.signbit(d) & (d == 0)).any() and (~np.signbit(d) & (d == 0)).any()
        ext = m.special_cols("int64_extremes", 1000, 12).values
        assert ext.max() == 2 ** 63 - 1 and ext.min() == -2 ** 63

    def test_partition_shapes(self):
        m = self.mx()
        k = m.source_constants()
        assert (k["PCHUNK"], k["MAX_PARTS"]) == (m.PCHUNK, m.MAX_PARTS)
        assert k["RETIRED"] == 2
        shapes = m.partition_shapes()
        assert len(shapes) == len(set(shapes)) == 48
        assert set(shapes) == {(n, p) for n in (0, 1, 64, 65, k["PCHUNK"] - 1, k["PCHUNK"],
                                                k["PCHUNK"] + 1, 2 * k["PCHUNK"] + 1)
                               for p in (1, 2, 63, 64, 65, k["MAX_PARTS"])}

    def test_ref_split_is_stable_and_uses_the_oracle(self):
        m = self.mx()
        cols = m.part_cols(500, 3)
        pids = m.ref_partition_ids(cols[:1], 7)
        h = oracle.hash_rows([cols[0].values], [oracle.TG_BIGINT])
        assert pids.tolist() == [oracle.partition_remote(int(np.int64(x)), 7) for x in h]
        parts = m.ref_split(pids, 7)
        assert sorted(i for p in parts for i in p) == list(range(500))
        assert all(p == sorted(p) for p in parts)
        assert all(pids[i] == q for q, p in enumerate(parts) for i in p)


class TestTextDistinctMatrixHost:
    """Host-side checks for tests/test_gpu_text_distinct_matrix.py: the
    references give hand-written verdicts (ref_like also agrees with
    re.fullmatch on the exhaustive set), every LIKE case expects both
    verdicts, the constants the shapes rest on equal the ones parsed from the
    sources, and each shape reaches the path it names. No GPU."""

    @staticmethod
    def mx():
        import test_gpu_text_distinct_matrix as m
        return m

    def test_ref_like_equals_re_fullmatch(self):
        import re
        m = self.mx()
        pats, texts = m.like_exhaustive_set()
        assert len(pats) == 364 and len(texts) == 427
        for p in pats:
            rx = re.compile(b".*".join(re.escape(s) for s in p.split(b"%")), re.S)
            for t in texts:
                assert m.ref_like(p, t) == (1 if rx.fullmatch(t) else 0), (p, t)

    def test_ref_like_by_hand(self):
        m = self.mx()
        for p, t, v in m.ANCHOR_BY_HAND + (
                (b"abc", b"abcd", 0), (b"abc", b"abc", 1), (b"abc", b"xabc", 0),   # L1
                (b"", b"", 1), (b"", b"a", 0), (b"%", b"a", 1), (b"%%", b"", 1),   # L2
                (b"a%b%c", b"abc", 1), (b"a%b%c", b"acb", 0), (b"a%c", b"ac", 1),
                (b"%\xc3\xa9%", b"a\xc3\xa9", 1), (b"%\xc3\xa9%", b"\xc3a\xa9", 0),
                (b"%a%", b"\x00a\x00", 1)):
            assert m.ref_like(p, t) == v, (p, t)

    def test_constants_follow_the_sources(self):
        m = self.mx()
        k = m.source_constants()
        assert (k["LIKE_MAX_SEGS"], k["LIKE_MAX_PAT"]) == (4, 64) == \
            (m.LIKE_MAX_SEGS, m.LIKE_MAX_PAT)
        assert (k["TG_BLOCK"], k["TG_MAX_BLOCKS"]) == (256, 2048)
        assert k["TG_BLOCK"] * k["TG_MAX_BLOCKS"] == m.GRID_THREADS
        assert m.GRID_N == m.GRID_THREADS + 257 == 524_545
        assert 1 << k["SORTED_SWITCH_SHIFT"] == m.SORTED_SWITCH == 1 << 20
        assert len(m.pool_bytes()) <= 1 << k["SORTED_KEY_BITS"]   # offsets fit the sort
        assert 1 << k["INIT_GROUPS_SHIFT"] == m.INIT_GROUPS == 1 << 16
        assert 1 << k["INIT_CAP_SHIFT"] == m.INIT_CAP == 1 << 17
        assert k["LOAD_FACTOR"] == m.LOAD_FACTOR == 0.7
        # the limits cases sit on the limits
        acc = m.like_case("limits_accepted")[1]
        assert max(p.count(b"%") + 1 for p in acc if not p.startswith(b"%")) == \
            m.LIKE_MAX_SEGS
        assert max(len(p) for p in acc) == m.LIKE_MAX_PAT - 1
        rej = m.LIKE_REJECTED
        assert any(len(p) == m.LIKE_MAX_PAT and b"_" not in p and b"%" not in p
                   for p in rej)
        assert any(len([s for s in p.split(b"%") if s]) == m.LIKE_MAX_SEGS + 1
                   and b"_" not in p for p in rej)
        assert all(b"_" in p or len(p) >= m.LIKE_MAX_PAT or
                   len([s for s in p.split(b"%") if s]) > m.LIKE_MAX_SEGS
                   for p in rej)

    def test_every_varchar_like_case_has_both_verdicts(self):
        m = self.mx()
        names = [c[0] for c in m.varchar_like_cases()]
        assert names == ["no_percent", "empty_pattern", "anchor_matrix",
                         "swar_lanes", "bytes_not_chars", "limits_accepted",
                         "grid_stride"]
        for name, patterns, rows in m.varchar_like_cases():
            for p in patterns:
                exp = [m.ref_like(p, t) for t in rows]
                if p in m.LIKE_ALL_ONE:
                    assert all(exp), (name, p)
                else:
                    assert 0 < sum(exp) < len(exp), (name, p)
        anchor_rows = m.like_case("anchor_matrix")[2]
        assert all(t in anchor_rows for _, t, _ in m.ANCHOR_BY_HAND)
        assert set(m.all_strings(b"abc", 5)) <= set(anchor_rows)
        assert set(m.ANCHOR_PATTERNS) >= {
            b"abc", b"abc%", b"%abc", b"%abc%", b"a%c", b"a%b%c", b"%a%b",
            b"a%b%", b"ab%ab", b"%", b"%%", b"%%a%%"}

    def test_swar_rows_cover_every_alignment_and_position(self):
        m = self.mx()
        texts = m.swar_texts()
        rows = m.rows_at_every_alignment(texts)
        seen, at = {}, 0
        for t in rows:
            seen.setdefault(t, set()).add(at % 8)
            at += len(t)
        for t in texts:
            assert seen[t] == set(range(8)), t
        for L in range(2, 41):
            for pos in range(L - 1):               # pos == L - 2: the last legal start
                for near in m.SWAR_NEAR:
                    hits = [t for t in texts if len(t) == L and
                            t.find(m.SWAR_SEG) == pos and
                            (near is None or pos == 0 or t.startswith(near[:1]))]
                    assert hits, (L, pos, near)
        near = {bytes([ord("Q") ^ 1]), bytes([ord("Q") ^ 0x80]), b"\x00", b"\xff", b"Qy"}
        assert near == {x for x in m.SWAR_NEAR if x}
        rows = m.like_case("grid_stride")[2]
        assert len(rows) == m.GRID_N and max(map(len, rows)) == 12
        assert rows[0] == rows[-1] == rows[m.GRID_THREADS] == b""

    def test_pool_cases(self):
        m = self.mx()
        pool = m.pool_bytes()
        P = len(pool)
        assert P == 300 * 1024 * 1024
        for offs, lens in (m.pool_constructed_slices(), m.pool_switch_slices()):
            assert offs.dtype == np.int64 and lens.dtype == np.int32
            assert offs.min() >= 0 and lens.min() >= 0
            assert int((offs + lens).max()) <= P
        offs, lens = m.pool_constructed_slices()
        assert int((offs + lens).max()) == P and int(offs.min()) == 0
        assert (lens == 0).any()
        assert len(offs) >= m.N_POOL_RANDOM
        assert pool.find(m.POOL_NOWHERE.strip(b"%")) == -1
        for p in m.POOL_PATTERNS:
            exp = m.pool_constructed_expected(p)
            if p == m.POOL_NOWHERE:
                assert not exp.any()
            else:
                assert m.both_verdicts(exp), p
        # the hand-built slices do what their comments say
        w = m.POOL_WORDS[0]
        o = m.occurrences(pool, w, 1, start=64)[0]
        sl = list(zip(offs.tolist(), lens.tolist()))
        i = sl.index((o - 10, 10 + len(w)))
        assert m.ref_like(b"%" + w, pool[o - 10:o + len(w)]) == 1
        assert m.ref_like(b"%" + w + b"%", pool[o - 10:o + len(w) - 1]) == 0
        assert sl[i + 1] == (o - 10, 10 + len(w) - 1)
        assert sl[i + 4] == (o, len(w)) and m.ref_like(w, pool[o:o + len(w)]) == 1
        # anchored, exact and '' patterns cannot take the index in mode 1
        assert set(m.POOL_FLOATING) | {m.POOL_NOWHERE} == {
            p for p in m.POOL_PATTERNS if p[:1] == b"%" and p[-1:] == b"%"
            and p.strip(b"%")}
        # default switch: duplicates of one offset with different verdicts
        offs, lens = m.pool_switch_slices()
        assert len(offs) == m.SORTED_SWITCH
        exp = m.pool_switch_expected()
        assert m.both_verdicts(exp) and m.both_verdicts(exp[:-1])
        by_off = {}
        for o_, l_, e_ in zip(offs.tolist(), lens.tolist(), exp.tolist()):
            by_off.setdefault(o_, set()).add((l_, e_))
        mixed = [v for v in by_off.values()
                 if {e for _, e in v} == {0, 1} and len({l for l, _ in v}) >= 4]
        assert len(mixed) >= 50

    def test_ref_mark_distinct_by_hand(self):
        m = self.mx()
        nan2 = float.fromhex("nan")
        rows = [(None, 1), (None, 2), (None, None), (None, 1), (1, None),
                (None, None)]
        assert m.ref_mark_distinct(rows) == [1, 1, 1, 0, 1, 0]
        rows = [(0.0,), (-0.0,), (math.nan,), (nan2,), (-math.nan,), (math.inf,),
                (-math.inf,), (None,), (math.inf,)]
        assert m.ref_mark_distinct(rows) == [1, 0, 1, 0, 0, 1, 1, 1, 0]
        rows = [(b"",), (None,), (b"a",), (b"ab",), (b"ac",), (b"",), (b"ab",),
                (b"\x00",)]
        assert m.ref_mark_distinct(rows) == [1, 1, 1, 1, 1, 0, 0, 1]
        assert m.ref_mark_distinct([(), (), ()]) == [1, 0, 0]
        # the double key column really holds the named values
        v = m.double_key_values(64, 1)
        bits = v.view(np.uint64).tolist()
        assert set(m.NAN_PAYLOADS) <= set(bits) and any(b >> 63 for b in m.NAN_PAYLOADS)
        assert 0 in bits and 1 << 63 in bits                       # 0.0 and -0.0
        assert math.inf in v.tolist() and -math.inf in v.tolist()
        s = m.varchar_key_values(64, 1)
        assert b"" in s and b"abc" in s and b"abd" in s and b"ab" in s

    def test_ref_partial_state_by_hand(self):
        m = self.mx()
        f = m.ref_partial_state
        one = m.f64_bits(1.0)
        assert f(m.FN_COUNT_STAR, None) == (1,) and f(m.FN_COUNT_STAR, 5) == (1,)
        assert f(m.FN_COUNT_COL, None) == (0,) and f(m.FN_COUNT_COL, -5) == (1,)
        assert f(m.FN_SUM_I64, None) == (0,) and f(m.FN_SUM_I64, -5) == (-5,)
        assert f(m.FN_SUM_F64, None) == (0,) and f(m.FN_SUM_F64, 1.0) == (one,)
        assert f(m.FN_MIN_I64, None) == (2 ** 63 - 1,) and f(m.FN_MIN_I64, 7) == (7,)
        assert f(m.FN_MAX_I64, None) == (-2 ** 63,) and f(m.FN_MAX_I64, 7) == (7,)
        assert f(m.FN_AVG_F64, None) == (0, 0) and f(m.FN_AVG_F64, 1.0) == (1, one)
        assert f(m.FN_SUM_F64_EXACT, None, 10) == (0, 0)
        assert f(m.FN_SUM_F64_EXACT, 1.5, 10) == (1536, 0)
        assert f(m.FN_SUM_F64_EXACT, -1.5, 10) == (-1536, -1)      # two's complement
        assert f(m.FN_SUM_F64_EXACT, 2.0 ** -10, 10) == (1, 0)

    def test_growth_and_page_shapes(self):
        m = self.mx()
        pages = m.mark_growth_pages()
        assert len(pages) == 3
        seen, before = set(), []
        for p in pages:
            keys = p[0].values.tolist()
            before.append((len(seen), len(keys)))
            seen |= set(keys)
        assert [b for b, _ in before] == [0, m.GROWTH_NEW, 2 * m.GROWTH_NEW]
        (g1, n1), (g2, n2), (g3, n3) = before
        cap07 = int(m.INIT_CAP * m.LOAD_FACTOR)
        assert g1 + n1 <= m.INIT_GROUPS and g1 + n1 <= cap07       # page 1: no growth
        assert g2 + n2 > m.INIT_GROUPS and g2 + n2 <= cap07        # page 2: key store
        assert g3 + n3 > cap07 and g3 + n3 <= 2 * m.INIT_GROUPS    # page 3: slot table
        assert set(pages[1][0].values.tolist()) & set(pages[0][0].values.tolist())
        assert m.PA_BITMAP_NS == (63, 64, 65, 129)
        assert len(m.mark_multi_case(7)[0]) == 8                    # 7 keys + 1 value
        # dedup: keys fit their width, the ends are present
        for name, keys, bits in m.dedup_cases():
            if len(keys):
                assert 0 <= int(keys.min()) and int(keys.max()) < 2 ** min(bits, 63), name
        ends = {b: k for n_, k, b in m.dedup_cases() if n_.startswith("ends_")}
        assert sorted(ends) == [1, 8, 31, 32, 33, 52, 64]
        for b, k in ends.items():
            assert set(k.tolist()) == {0, 2 ** min(b, 63) - 1}
        sizes = {len(k) for _, k, _ in m.dedup_cases()}
        assert {0, 1, 2, m.GRID_N, (1 << 20) + 3} <= sizes
