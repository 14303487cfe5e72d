/* ops_join.hip — hash join build + probe (nonspilling).
 *
 * Mirrors:
 *  - build: operator/join/nonspilling/HashBuilderOperator.java:140-380 state
 *    machine (CONSUMING_INPUT -> LOOKUP_SOURCE_BUILT), PagesIndex.java:91-92
 *    page accumulation with synthetic addresses (SyntheticAddress.java:26-29:
 *    (sliceIndex<<32)|position), BigintPagesHash.java:62-143 (single BIGINT
 *    key: values copied to a flat array, open addressing, murmur3 position,
 *    PagesHash.java:35-51), sizing IncrementalLoadFactorHashArraySizeSupplier
 *    .java:26-45 (0.25/0.5/0.75), duplicate keys chained through
 *    ArrayPositionLinks.java:24-45 (links[new]=old, new row becomes head).
 *    The default CSR build sorts each bucket by build row and the probe
 *    walks buckets descending, reproducing the reference's reverse-insertion
 *    duplicate order deterministically at every size. (The legacy
 *    open-addressing path, TG_JOIN_CSR=0, pushes chains with atomicExch and
 *    is only deterministic for single-workgroup builds.)
 *  - probe: LookupJoinOperator / DefaultPageJoiner.java:243-296 +
 *    JoinProbe.java:112-180 batch shape and DefaultPagesHash.java:193-280
 *    (hash all -> gather all -> verify -> probe misses); null keys never
 *    match; per probe row the head match is emitted then the chain is walked.
 *    Output assembly mirrors LookupJoinPageBuilder.java:89-119: probe columns
 *    gathered by probe position, build columns gathered by synthetic address.
 *  - join filter: JoinFilterFunction.filter(left, right, page), which the
 *    reference tests on every position of the link chain; here one step
 *    (LookupJoinOp::filter_matches) on the candidate list every probe path
 *    ends in, before the visited marks and the gathers.
 */
#include "dev_hash.h"
#include "expr_eval.h"

/* inline single-entry bucket (the common case: unique build keys): one
 * aligned 16-byte random read resolves most probes instead of three
 * (bucket_off, csr_rows, keys). row -1 = empty bucket, -2 = bucket with
 * >1 rows (fall back to the CSR walk). Built for single-BIGINT-key tables. */
struct SlotKV {
    int64_t key;
    int32_t row;
    int32_t _pad;
};

struct JoinTable {
    int64_t n = 0;               /* build rows */
    int64_t capacity = 0, mask = 0;
    int32_t csr = 0;             /* 1 = CSR bucket index (no probing) */
    int32_t* slots = nullptr;    /* open addressing: -1 empty else row index */
    int32_t* links = nullptr;    /* open addressing: dup chain */
    /* CSR mode: bucket b(=slot) holds rows csr_rows[bucket_off[b] ..
     * bucket_off[b+1]); different keys hashing to one slot share the bucket
     * and are filtered by the key compare (no linear probing). */
    int32_t* bucket_off = nullptr;  /* [capacity+1] */
    int32_t* csr_rows = nullptr;    /* [n] */
    int64_t* csr_keys = nullptr;    /* [n] keys in bucket order (single-key
                                       tables): the probe compare reads one
                                       slot-local line instead of the random
                                       csr_rows -> keys chain */
    int64_t* keys = nullptr;     /* [n] flat copy of build keys */
    uint64_t* key_valid = nullptr; /* packed bitmap or null */
    /* generic multi-channel keys (DefaultPagesHash analog; the fields above
     * are the BigintPagesHash specialization). bkeys points at the bridge's
     * concatenated build channels. */
    int32_t generic = 0;
    int32_t n_key_ch = 1;
    const KColH* bkeys = nullptr;   /* device array[n_key_ch] */
    const SlotKV* kv = nullptr;     /* single-key fast table or null */
    int32_t has_null_key = 0;       /* any build key row null (semi-join 3VL) */
    /* ChannelSet analog (SetBuilderOperator.java): dense-range bitmap for
     * semi-join membership — no positions, no chains */
    const uint64_t* set_bitmap = nullptr;
    int64_t set_min = 0, set_max = 0;
};

/* slot of a build row; generic keys hash with the canonical row hash
 * (InterpretedHashGenerator semantics) finalized by murmur3, like
 * DefaultPagesHash.getHashPosition over strategy raw hashes */
__device__ static inline uint32_t jt_build_slot(const JoinTable& t, int64_t row)
{
    uint64_t h = t.generic ? row_hash(t.bkeys, t.n_key_ch, row)
                           : (uint64_t)t.keys[row];
    return (uint32_t)(d_murmur3_mix(h) & (uint64_t)t.mask);
}

__device__ static inline bool jt_build_null(const JoinTable& t, int64_t row)
{
    if (!t.generic)
        return t.key_valid && !((t.key_valid[row >> 6] >> (row & 63)) & 1);
    for (int c = 0; c < t.n_key_ch; c++)
        if (kcol_is_null(t.bkeys[c], row)) return true;
    return false;
}

/* probe-side context: fast single-bigint pointer OR generic channel array */
struct ProbeKeys {
    const int64_t* pk = nullptr;
    const uint64_t* pvalid = nullptr;
    const KColH* pkg = nullptr;   /* device array[n_key_ch] when generic */
};

__device__ static inline bool probe_null(const JoinTable& t, const ProbeKeys& p, int64_t i)
{
    if (!t.generic)
        return p.pvalid && !((p.pvalid[i >> 6] >> (i & 63)) & 1);
    for (int c = 0; c < t.n_key_ch; c++)
        if (kcol_is_null(p.pkg[c], i)) return true;
    return false;
}

__device__ static inline uint32_t probe_slot(const JoinTable& t, const ProbeKeys& p, int64_t i)
{
    uint64_t h = t.generic ? row_hash(p.pkg, t.n_key_ch, i) : (uint64_t)p.pk[i];
    return (uint32_t)(d_murmur3_mix(h) & (uint64_t)t.mask);
}

__device__ static inline bool probe_matches(const JoinTable& t, const ProbeKeys& p,
                                            int64_t probe_row, int32_t build_row)
{
    if (!t.generic) return t.keys[build_row] == p.pk[probe_row];
    for (int c = 0; c < t.n_key_ch; c++) {
        const KColH& bc = t.bkeys[c];
        const KColH& pc = p.pkg[c];
        if (bc.type == TG_VARCHAR) {   /* VarcharType EQUAL: byte equality */
            int32_t bo = bc.offsets[build_row];
            int32_t bl = bc.offsets[build_row + 1] - bo;
            int32_t po = pc.offsets[probe_row];
            if (bl != pc.offsets[probe_row + 1] - po) return false;
            const uint8_t* bb = (const uint8_t*)bc.data + bo;
            const uint8_t* pb = (const uint8_t*)pc.data + po;
            for (int32_t k = 0; k < bl; k++)
                if (bb[k] != pb[k]) return false;
        }
        else if (bc.type == TG_DOUBLE) {
            /* the join criterion `=` is IEEE ==: -0.0 matches 0.0 and NaN
             * matches nothing (the canonical word is the GROUPING identity,
             * where every NaN is one value; the hash stays canonical, so
             * equal doubles still share a slot) */
            if (!(((const double*)bc.data)[build_row] ==
                  ((const double*)pc.data)[probe_row]))
                return false;
        }
        else if (kcol_word(bc, build_row) != kcol_word(pc, probe_row))
            return false;
    }
    return true;
}

struct tg_join_bridge {
    tg_session* s;
    /* owner of every device buffer that lives as long as the bridge: the
     * table arrays of `t`, set_bitmap, kv, d_bkeys, visited and the data,
     * valid and offsets of build_channels. The fields that point at them stay
     * plain pointers (JoinTable goes to kernels by value); closing the bridge
     * frees them all. */
    PoolScratch own;
    explicit tg_join_bridge(tg_session* s_) : s(s_), own(s_) {}
    JoinTable t;
    /* dynamic filter source (DynamicFilterSourceOperator /
     * sql/gen/columnar/DynamicPageFilter.java analog): min/max of the
     * non-null build keys, collected at build finish and pushed into the
     * probe-side scan filter by the pipeline driver */
    int64_t key_min = 0, key_max = 0;
    int64_t key_rows = 0;
    /* concatenated build output channels (contiguous by global build row) */
    std::vector<DevBlock> build_channels;
    std::vector<tg_type> build_types;
    std::vector<int32_t> build_output_channels;
    std::vector<int32_t> key_channels;
    KColH* d_bkeys = nullptr;        /* device array over build key channels */
    bool built = false;
    /* fused dynamic filter (DynamicPageFilter.java analog): when requested
     * BEFORE build finish, a dense-range key membership bitmap is built
     * alongside the index and pushed into probe-side scan kernels. Best
     * effort like the reference: generic keys / huge ranges skip it. */
    bool want_bitmap = false;
    /* build-outer (RIGHT / FULL) bookkeeping, the JoinBridge outer-position
     * tracker analog: one visited bit per global build row, allocated and
     * zeroed when the first recording probe operator (join_type 2 or 3) adds
     * a page; `recording` counts such operators created and not yet finished
     * or closed; `plain_probed` is set once a join_type 0 or 1 operator has
     * probed, after which the visited set can no longer be complete. */
    uint64_t* visited = nullptr;     /* [ceil(n / 64)] */
    int32_t recording = 0;
    bool plain_probed = false;
};

/* a bridge the positional operators cannot serve: the set builder's bitmap
 * holds membership only, no rows */
static bool bridge_is_set_only(const tg_join_bridge* b)
{
    return b->t.set_bitmap && !b->t.csr;
}

/* probe-side key channels must mirror the build's: same count and, per
 * position, the same type. The probe kernels index the probe KColH array by
 * the BUILD's channel count and pick the compare by the BUILD's type, so a
 * mismatch would read past the array or through null VARCHAR offsets. */
static tg_status check_probe_keys(const tg_join_bridge* b, const tg_page* page,
                                  const int32_t* key_channels, size_t n_keys)
{
    if (n_keys != b->key_channels.size()) {
        TG_SET_ERR("probe has %zu join key channels, the build has %zu",
                   n_keys, b->key_channels.size());
        return TG_ERR_INVALID_ARG;
    }
    for (size_t k = 0; k < n_keys; k++) {
        int32_t ch = key_channels[k];
        if (ch < 0 || ch >= page->channel_count) {
            TG_SET_ERR("probe join key channel %d outside the page's %d channels",
                       ch, page->channel_count);
            return TG_ERR_INVALID_ARG;
        }
        int32_t bt = (int32_t)b->build_types[b->key_channels[k]];
        int32_t pt = (int32_t)page->blocks[ch].type;
        if (bt != pt) {
            TG_SET_ERR("join key %zu type mismatch: probe channel %d has type %d, "
                       "the build key has type %d", k, ch, pt, bt);
            return TG_ERR_INVALID_ARG;
        }
    }
    return TG_OK;
}

/* probe-side key context over an uploaded page: the BIGINT key pointers, or
 * for generic keys a device KColH array that `scratch` owns */
static tg_status probe_keys_of(tg_session* s, const JoinTable& t, const DevPage& in,
                               const int32_t* channels, int n_channels,
                               PoolScratch& scratch, ProbeKeys* pkc)
{
    if (t.generic) {
        KColH* d_pkg = nullptr;
        tg_status st = make_kcols(s, in, channels, n_channels, &d_pkg);
        scratch.adopt(d_pkg);     /* also when the copy after its allocation failed */
        pkc->pkg = d_pkg;
        return st;
    }
    const DevBlock& kb = in.blocks[channels[0]];
    if (kb.type != TG_BIGINT) { TG_SET_ERR("single join key must be BIGINT (use multi-channel keys otherwise)"); return TG_ERR_UNSUPPORTED; }
    pkc->pk = (const int64_t*)kb.data;
    pkc->pvalid = kb.valid;
    return TG_OK;
}

/* IncrementalLoadFactorHashArraySizeSupplier (multiplier 1) */
static int64_t join_hash_size(int64_t expected)
{
    double f = expected <= (1 << 16) ? 0.25 : expected <= (1 << 20) ? 0.50 : 0.75;
    int64_t need = (int64_t)(expected / f);
    if (need < 2) need = 2;
    int64_t cap = 1;
    while (cap < need) cap <<= 1;
    return cap;
}

__global__ void k_join_init(int32_t* slots, int64_t cap, int32_t* links, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = i; k < cap; k += stride) slots[k] = -1;
    for (int64_t k = i; k < n; k += stride) links[k] = -1;
}

__global__ void k_key_minmax(const int64_t* __restrict__ keys,
                             const uint64_t* __restrict__ valid, int64_t n,
                             long long* mn, long long* mx, unsigned long long* cnt)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    long long lmn = INT64_MAX, lmx = INT64_MIN;
    unsigned long long lc = 0;
    for (; i < n; i += stride) {
        if (valid && !((valid[i >> 6] >> (i & 63)) & 1)) continue;
        long long v = keys[i];
        lmn = min(lmn, v); lmx = max(lmx, v); lc++;
    }
    /* block-free: atomics are fine here (once per lane per launch) */
    atomicMin(mn, lmn);
    atomicMax(mx, lmx);
    atomicAdd(cnt, lc);
}

/* ---- CSR build: count -> per-region LDS exclusive scan -> parallel
 * atomic scatter -> per-bucket sort by build row. Replaces the global
 * atomic-CAS insert (measured ~1 G CAS/s = 15 ms per 15M-row build) and
 * the earlier chunk-ordered scatter (serial per chunk with a global-memory
 * cursor RMW per row: 16 ms/step on Q3 SF100). The ascending in-bucket sort
 * plus the descending probe walk reproduces ArrayPositionLinks' reverse-
 * insertion duplicate order (ArrayPositionLinks.java:24-45) DETERMINISTICALLY
 * at every size. ---- */
#define JREG_SLOTS 32768              /* slots per region (LDS u32 counts) */

__global__ void k_jc_count(JoinTable t, uint32_t* __restrict__ slot_of,
                           int32_t* __restrict__ bucket_cnt /* zeroed [cap] */)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < t.n; i += stride) {
        bool null = jt_build_null(t, i);
        uint32_t slot = null ? 0xFFFFFFFFu : jt_build_slot(t, i);
        slot_of[i] = slot;
        if (!null) atomicAdd(&bucket_cnt[slot], 1);
    }
}

__global__ __launch_bounds__(TG_BLOCK)
void k_jc_local_off(const int32_t* __restrict__ bucket_cnt,
                    int32_t* __restrict__ bucket_off,
                    int32_t* __restrict__ region_total,
                    int64_t nreg, int64_t region_slots)
{
    /* one block per region: region-local exclusive prefix of the per-slot
     * counts (LDS staged; region_slots <= JREG_SLOTS = 128 KB of u32) */
    int64_t reg = blockIdx.x;
    if (reg >= nreg) return;
    __shared__ int32_t cnt[JREG_SLOTS];
    __shared__ int32_t wpart[TG_BLOCK / 64];
    int64_t sbase = reg * region_slots;
    const int per = (int)((region_slots + blockDim.x - 1) / blockDim.x);
    int32_t mysum = 0;
    for (int k = 0; k < per; k++) {
        int64_t sidx = (int64_t)threadIdx.x * per + k;
        if (sidx < region_slots) {
            int32_t v = bucket_cnt[sbase + sidx];
            cnt[sidx] = v;
            mysum += v;
        }
    }
    int32_t wpre = mysum;
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int32_t o = __shfl_up(wpre, off, 64);
        if ((int)(threadIdx.x % 64) >= off) wpre += o;
    }
    if (threadIdx.x % 64 == 63) wpart[threadIdx.x / 64] = wpre;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t run = 0;
        for (int w = 0; w < (int)(blockDim.x / 64); w++) {
            int32_t v = wpart[w];
            wpart[w] = run;
            run += v;
        }
        region_total[reg] = run;
    }
    __syncthreads();
    int32_t base = wpart[threadIdx.x / 64] + wpre - mysum;
    for (int k = 0; k < per; k++) {
        int64_t sidx = (int64_t)threadIdx.x * per + k;
        if (sidx >= region_slots) break;
        int32_t v = cnt[sidx];
        bucket_off[sbase + sidx] = base;
        base += v;
    }
}

__global__ void k_jc_addbase(int32_t* __restrict__ bucket_off, int64_t capacity,
                             const int32_t* __restrict__ region_base,
                             int64_t region_slots)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < capacity; i += stride)
        bucket_off[i] += region_base[i / region_slots];
}

__global__ void k_jc_scatter(JoinTable t, const uint32_t* __restrict__ slot_of,
                             int32_t* __restrict__ cursor /* copy of bucket_off */)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < t.n; i += stride) {
        uint32_t slot = slot_of[i];
        if (slot == 0xFFFFFFFFu) continue;      /* null key: never indexed */
        int32_t at = atomicAdd(&cursor[slot], 1);
        t.csr_rows[at] = (int32_t)i;
    }
}

__global__ void k_jc_sort(JoinTable t)
{
    /* ascending insertion sort within each bucket (expected length n/cap
     * < 1; the tail is a handful of duplicates sharing a slot) */
    int64_t s0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t sl = s0; sl < t.capacity; sl += stride) {
        int32_t lo = t.bucket_off[sl], hi = t.bucket_off[sl + 1];
        for (int32_t a = lo + 1; a < hi; a++) {
            int32_t v = t.csr_rows[a];
            int32_t b = a - 1;
            for (; b >= lo && t.csr_rows[b] > v; b--) t.csr_rows[b + 1] = t.csr_rows[b];
            t.csr_rows[b + 1] = v;
        }
    }
}

__global__ void k_csr_keys(JoinTable t, int64_t* __restrict__ ck)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t tot = t.bucket_off[t.capacity];   /* indexed rows (null keys excluded) */
    for (; i < tot; i += stride) ck[i] = t.keys[t.csr_rows[i]];
}

__global__ void k_build_slotkv(JoinTable t, SlotKV* __restrict__ kv)
{
    int64_t s0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t sl = s0; sl < t.capacity; sl += stride) {
        int32_t lo = t.bucket_off[sl], hi = t.bucket_off[sl + 1];
        SlotKV e;
        if (hi - lo == 1) { e.row = t.csr_rows[lo]; e.key = t.keys[e.row]; }
        else { e.row = (hi == lo) ? -1 : -2; e.key = 0; }
        e._pad = 0;
        kv[sl] = e;
    }
}

__global__ void k_set_bits(const int64_t* __restrict__ keys,
                           const uint64_t* __restrict__ valid, int64_t n,
                           int64_t base, uint64_t* __restrict__ bm)
{
    /* wave-segmented: clustered keys (lineitem orderkeys) put many lanes in
     * the same bitmap WORD — OR-combine per equal-word run in registers and
     * let only the run's last lane issue the atomic (Q4's 380M-key build:
     * per-lane check-then-set atomics measured 18.3 ms, ~10x the traffic) */
    int lane = threadIdx.x % 64;
    int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t iw = i0 - lane; iw < n; iw += stride) {
        int64_t i = iw + lane;
        bool active = i < n &&
                      !(valid && !((valid[i >> 6] >> (i & 63)) & 1));
        int64_t w = -1;
        uint64_t bit = 0;
        if (active) {
            uint64_t k = (uint64_t)(keys[i] - base);
            w = (int64_t)(k >> 6);
            bit = 1ull << (k & 63);
        }
        /* inclusive OR-scan over equal-w prefixes */
        #pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            uint64_t ob = __shfl_up(bit, off, 64);
            int64_t ow = __shfl_up(w, off, 64);
            if (lane >= off && ow == w) bit |= ob;
        }
        int64_t wnext = __shfl_down(w, 1, 64);
        bool last = active && (lane == 63 || i + 1 >= n || wnext != w);
        if (last && (bm[w] & bit) != bit)
            atomicOr((unsigned long long*)&bm[w], (unsigned long long)bit);
    }
}

__global__ void k_join_build(JoinTable t)
{
    /* Probe with PLAIN loads and resolve races with device-scope atomics:
     * a stale -1 is corrected by the CAS (which returns the real occupant),
     * and a slot's occupant KEY identity never changes after the first claim
     * (only equal-key rows are exchanged in), so a stale occupant row index
     * still compares the right key. Agent-scope atomic LOADS per probe step
     * bypass the caches and measured 15 ms per 15M-row build; plain loads
     * with CAS fallback are ~an order of magnitude cheaper. */
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < t.n; i += stride) {
        if (t.key_valid && !((t.key_valid[i >> 6] >> (i & 63)) & 1)) continue;
        int64_t key = t.keys[i];
        int64_t slot = (int64_t)(d_murmur3_mix((uint64_t)key) & (uint64_t)t.mask);
        while (true) {
            int32_t cur = *(volatile int32_t*)&t.slots[slot];
            if (cur == -1) {
                int32_t expected = -1;
                if (__hip_atomic_compare_exchange_strong(&t.slots[slot], &expected,
                        (int32_t)i, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT))
                    break;
                cur = expected;
            }
            if (t.keys[cur] == key) {
                /* chain push: links[mine] = previous head (ArrayPositionLinks) */
                int32_t prev = __hip_atomic_exchange(&t.slots[slot], (int32_t)i,
                        __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
                t.links[i] = prev;
                break;
            }
            slot = (slot + 1) & t.mask;
        }
    }
}

/* probe phase 1 (DefaultPagesHash.getAddressIndex hash-all/gather-all/verify
 * shape): count matches per probe row, caching the matched head so the fill
 * pass never re-probes the table */
/* ---- partitioned single-pass probe (large single-BIGINT-key tables) ----
 * The two-pass count/fill walk reads 2-3 random cache lines per probe over a
 * table far larger than L2. Instead: bucket-partition the PROBE ROWS by slot
 * region (so consecutive rows hit a table slice that stays cache-resident),
 * walk each bucket once appending (probe_row, build_row) matches, then
 * restore probe-row order with a stable radix sort — the reference emits
 * matches in probe position order (DefaultPageJoiner), duplicates in
 * reverse-insertion order (descending walk + stable sort preserves it). */
__global__ void k_pb_slots(JoinTable t, ProbeKeys p, int64_t m, int64_t nparts,
                           int shift, uint32_t* __restrict__ slot_of,
                           int32_t* __restrict__ pcount)
{
    extern __shared__ int32_t lh[];
    for (int64_t k = threadIdx.x; k < nparts; k += blockDim.x) lh[k] = 0;
    __syncthreads();
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < m; i += stride) {
        uint32_t slot = probe_null(t, p, i) ? 0xFFFFFFFFu : probe_slot(t, p, i);
        slot_of[i] = slot;
        if (slot != 0xFFFFFFFFu) atomicAdd(&lh[slot >> shift], 1);
    }
    __syncthreads();
    for (int64_t k = threadIdx.x; k < nparts; k += blockDim.x)
        if (lh[k]) atomicAdd(&pcount[k], lh[k]);
}

__global__ void k_pb_scatter(JoinTable t, ProbeKeys p, int64_t m, int shift,
                             const uint32_t* __restrict__ slot_of,
                             int32_t* __restrict__ pcur, int64_t nparts,
                             uint32_t* __restrict__ pi, uint32_t* __restrict__ pslot,
                             int64_t* __restrict__ pkey)
{
    /* block-hierarchical: LDS per-partition counts -> one global reserve per
     * (block, partition) -> LDS-cursor scatter. A flat per-row atomicAdd on
     * the handful of partition cursors serialized the whole pass (measured
     * 1.3 s/step at 275M rows x 32 partitions). */
    extern __shared__ int32_t sh[];      /* [nparts] counts, then cursors */
    int64_t chunk = (m + gridDim.x - 1) / gridDim.x;
    int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(lo + chunk, m);
    for (int64_t k = threadIdx.x; k < nparts; k += blockDim.x) sh[k] = 0;
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        uint32_t slot = slot_of[i];
        if (slot != 0xFFFFFFFFu) atomicAdd(&sh[slot >> shift], 1);
    }
    __syncthreads();
    for (int64_t k = threadIdx.x; k < nparts; k += blockDim.x) {
        int32_t c = sh[k];
        sh[k] = c ? atomicAdd(&pcur[k], c) : 0;
    }
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        uint32_t slot = slot_of[i];
        if (slot == 0xFFFFFFFFu) continue;
        int32_t at = atomicAdd(&sh[slot >> shift], 1);
        pi[at] = (uint32_t)i;
        pslot[at] = slot;
        pkey[at] = p.pk[i];
    }
}

__global__ void k_pb_probe(JoinTable t, int64_t jlo, int64_t jhi,
                           const uint32_t* __restrict__ pi,
                           const uint32_t* __restrict__ pslot,
                           const int64_t* __restrict__ pkey,
                           unsigned long long* __restrict__ out_cnt,
                           int64_t cap,
                           uint32_t* __restrict__ mp, int32_t* __restrict__ mb)
{
    /* ONE LAUNCH PER PARTITION (host loop, stream-ordered): while this
     * launch runs, every bucket_off/csr_keys/csr_rows read lands in the
     * partition's ~16 MB table slice, which stays cache-resident.
     * DESCENDING walk + per-thread ordered appends + the later stable sort
     * by probe row = the reference's reverse-insertion duplicate order. */
    int64_t midx = jhi - jlo;
    int64_t chunk = (midx + gridDim.x - 1) / gridDim.x;
    int64_t lo = jlo + (int64_t)blockIdx.x * chunk, hi = min(lo + chunk, jhi);
    int lane = threadIdx.x % 64;
    /* wave-aggregated reservation: one atomicAdd per wave iteration instead
     * of one per match (a single global counter otherwise serializes) */
    for (int64_t j0 = lo + (threadIdx.x / 64) * 64; j0 < hi;
         j0 += (int64_t)(blockDim.x / 64) * 64 * 1) {
        int64_t j = j0 + lane;
        int32_t cnt = 0;
        uint32_t slot = 0; int64_t key = 0;
        int32_t blo = 0, bhi = 0;
        if (j < hi) {
            slot = pslot[j];
            key = pkey[j];
            blo = t.bucket_off[slot];
            bhi = t.bucket_off[slot + 1];
            for (int32_t x = bhi - 1; x >= blo; x--) cnt += (t.csr_keys[x] == key);
        }
        int32_t pre = cnt;
        #pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            int32_t o = __shfl_up(pre, off, 64);
            if (lane >= off) pre += o;
        }
        int32_t wave_total = __shfl(pre, 63, 64);
        unsigned long long base = 0;
        if (lane == 63 && wave_total)
            base = atomicAdd(out_cnt, (unsigned long long)wave_total);
        base = __shfl(base, 63, 64);
        if (j < hi && cnt) {
            int64_t pos = (int64_t)base + pre - cnt;
            for (int32_t x = bhi - 1; x >= blo; x--) {
                if (t.csr_keys[x] == key && pos < cap) {
                    mp[pos] = pi[j];
                    mb[pos] = t.csr_rows[x];
                    pos++;
                }
            }
        }
    }
}

__global__ void k_probe_count(JoinTable t, ProbeKeys p, int64_t m, int outer,
                              int32_t* __restrict__ counts,
                              int32_t* __restrict__ heads)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < m; i += stride) {
        int32_t cnt = 0;
        int32_t head = -1;
        /* empty build: nothing matches and there is no table to walk (a
         * generic-key probe has no pk for the legacy branch to read) */
        if (t.n > 0 && !probe_null(t, p, i)) {
            int64_t slot = (int64_t)probe_slot(t, p, i);
            if (t.kv) {          /* one 16B read resolves most probes */
                SlotKV e = t.kv[slot];
                if (e.row >= 0) {
                    head = (e.key == p.pk[i]) ? -2 - e.row : -1;
                    cnt = (head != -1);
                }
                else if (e.row == -1) head = -1;
                else {               /* multi-row bucket: CSR walk */
                    int32_t matched = -1;
                    for (int32_t x = t.bucket_off[slot]; x < t.bucket_off[slot + 1]; x++) {
                        int32_t row = t.csr_rows[x];
                        if (probe_matches(t, p, i, row)) { cnt++; matched = row; }
                    }
                    head = (cnt == 1) ? -2 - matched : (cnt == 0 ? -1 : (int32_t)slot);
                }
            }
            else if (t.csr && t.csr_keys) {   /* single-key: slot-local compare */
                int64_t key = p.pk[i];
                int32_t matched = -1;
                for (int32_t x = t.bucket_off[slot]; x < t.bucket_off[slot + 1]; x++) {
                    if (t.csr_keys[x] == key) { cnt++; matched = x; }
                }
                head = (cnt == 1) ? -2 - t.csr_rows[matched]
                                  : (cnt == 0 ? -1 : (int32_t)slot);
            }
            else if (t.csr) {
                int32_t matched = -1;
                for (int32_t x = t.bucket_off[slot]; x < t.bucket_off[slot + 1]; x++) {
                    int32_t row = t.csr_rows[x];
                    if (probe_matches(t, p, i, row)) { cnt++; matched = row; }
                }
                /* single match (the usual case: unique build keys): encode
                 * the row as -2-row so the fill pass skips the bucket walk */
                head = (cnt == 1) ? -2 - matched : (cnt == 0 ? -1 : (int32_t)slot);
            }
            else {   /* legacy open addressing: single-BIGINT only */
                int64_t key = p.pk[i];
                int32_t cur;
                while ((cur = t.slots[slot]) != -1) {
                    if (t.keys[cur] == key) {
                        head = cur;
                        for (int32_t q = cur; q != -1; q = t.links[q]) cnt++;
                        break;
                    }
                    slot = (slot + 1) & t.mask;
                }
            }
        }
        /* probe-outer (LEFT): unmatched rows (incl. null keys) emit one
         * row with a null build side (LookupJoinOperator probeOnOuterSide,
         * LookupJoinOperators.java) */
        if (outer && cnt == 0) { cnt = 1; head = INT32_MIN; }
        counts[i] = cnt;
        heads[i] = head;
    }
}

/* probe phase 2: emit (probe_row, build_row) pairs from the cached heads.
 * CSR: walk the bucket DESCENDING — scatter order is global row order, so
 * this reproduces ArrayPositionLinks' reverse-insertion emission exactly
 * (and deterministically). */
__global__ void k_probe_fill(JoinTable t, ProbeKeys p, int64_t m,
                             const int32_t* __restrict__ heads,
                             const int64_t* __restrict__ offsets,
                             int32_t* __restrict__ out_probe,
                             int32_t* __restrict__ out_build)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < m; i += stride) {
        int64_t at = offsets[i];
        int32_t h = heads[i];
        if (h == -1) continue;
        if (h == INT32_MIN) {    /* probe-outer miss: null build side */
            out_probe[at] = (int32_t)i;
            out_build[at] = -1;
            continue;
        }
        if (h <= -2) {           /* pre-resolved single match */
            out_probe[at] = (int32_t)i;
            out_build[at] = -2 - h;
            continue;
        }
        if (t.csr && t.csr_keys) {
            int64_t key = p.pk[i];
            for (int32_t x = t.bucket_off[h + 1] - 1; x >= t.bucket_off[h]; x--) {
                if (t.csr_keys[x] == key) {
                    out_probe[at] = (int32_t)i;
                    out_build[at] = t.csr_rows[x];
                    at++;
                }
            }
        }
        else if (t.csr) {
            for (int32_t x = t.bucket_off[h + 1] - 1; x >= t.bucket_off[h]; x--) {
                int32_t row = t.csr_rows[x];
                if (probe_matches(t, p, i, row)) {
                    out_probe[at] = (int32_t)i;
                    out_build[at] = row;
                    at++;
                }
            }
        }
        else {
            for (int32_t q = h; q != -1; q = t.links[q]) {
                out_probe[at] = (int32_t)i;
                out_build[at] = q;
                at++;
            }
        }
    }
}

/* two-level exclusive scan of per-row counts (n can be 10^8+):
 * chunk sums -> serial chunk scan -> per-row offsets within chunk */
#define JSCAN_CHUNK 65536
__global__ void k_scan_chunk_sums(const int32_t* __restrict__ counts, int64_t n,
                                  int64_t* __restrict__ chunk_sums, int64_t nchunks)
{
    /* one wave per chunk: lanes stride the chunk, shuffle-reduce */
    int64_t c = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (c >= nchunks) return;
    int lane = threadIdx.x % 64;
    int64_t lo = c * JSCAN_CHUNK, hi = min(lo + JSCAN_CHUNK, n);
    long long s = 0;
    for (int64_t i = lo + lane; i < hi; i += 64) s += counts[i];
    #pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) chunk_sums[c] = s;
}

__global__ void k_scan_chunks_serial(int64_t* chunk_sums, int64_t nchunks, int64_t* total)
{
    if (blockIdx.x || threadIdx.x) return;
    int64_t run = 0;
    for (int64_t i = 0; i < nchunks; i++) {
        int64_t v = chunk_sums[i];
        chunk_sums[i] = run;
        run += v;
    }
    *total = run;
}

__global__ void k_scan_row_offsets(const int32_t* __restrict__ counts, int64_t n,
                                   const int64_t* __restrict__ chunk_sums,
                                   int64_t* __restrict__ offsets, int64_t nchunks)
{
    /* one wave per chunk walks it carrying a running sum */
    int64_t c = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (c >= nchunks) return;
    int lane = threadIdx.x % 64;
    int64_t lo = c * JSCAN_CHUNK, hi = min(lo + JSCAN_CHUNK, n);
    int64_t run = chunk_sums[c];
    for (int64_t g = lo; g < hi; g += 64) {
        int64_t i = g + lane;
        long long v = (i < hi) ? counts[i] : 0;
        /* exclusive wave prefix via shuffles */
        long long pre = v;
        #pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            long long o = __shfl_up(pre, off, 64);
            if (lane >= off) pre += o;
        }
        long long wave_total = __shfl(pre, 63, 64);
        if (i < hi) offsets[i] = run + pre - v;
        run += wave_total;
    }
}

static tg_status run_scan_counts(tg_session* s, const int32_t* d_counts, int64_t n,
                                 int64_t* d_offsets, int64_t* d_total)
{
    int64_t nchunks = (n + JSCAN_CHUNK - 1) / JSCAN_CHUNK;
    if (nchunks < 1) nchunks = 1;
    PoolScratch scratch(s);
    int64_t* d_cs = nullptr;
    TG_TRY(scratch.alloc(&d_cs, nchunks * 8));
    int swpb = TG_BLOCK / 64;
    hipLaunchKernelGGL(k_scan_chunk_sums, dim3((uint32_t)((nchunks + swpb - 1) / swpb)),
                       dim3(TG_BLOCK), 0, s->stream, d_counts, n, d_cs, nchunks);
    TG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_scan_chunks_serial, dim3(1), dim3(1), 0, s->stream,
                       d_cs, nchunks, d_total);
    TG_HIP_CHECK(hipGetLastError());
    int wpb = TG_BLOCK / 64;
    hipLaunchKernelGGL(k_scan_row_offsets, dim3((uint32_t)((nchunks + wpb - 1) / wpb)),
                       dim3(TG_BLOCK), 0, s->stream, d_counts, n, d_cs, d_offsets, nchunks);
    TG_HIP_CHECK(hipGetLastError());
    TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    return TG_OK;
}

/* ---- build-outer (RIGHT / FULL): visited bitmap + unmatched-row emission
 * (LookupJoinOperators buildOuter / LookupOuterOperator.java: the probe
 * records the build positions it joined, the outer operator then emits the
 * positions nobody visited) ---- */

/* One pass over the matched build row list d_ob[0..total) that EVERY probe
 * path of LookupJoinOp::add_input ends with, so recording is independent of
 * the path that produced the list. -1 entries (FULL's probe-outer misses)
 * are skipped. Wave-segmented like k_set_bits, for the same reason: the list
 * is probe-row ordered, so a hot build row (millions of probes hitting one
 * row, or the 500 copies of one key walked in descending row order) fills
 * whole waves with the same bitmap WORD. Each equal-word run is OR-combined
 * in registers, only the run's last lane looks at memory, and it skips the
 * atomic when a plain load shows its bits already set (bits only ever go
 * 0 -> 1 while probing, so a stale 0 costs one redundant atomic, never a
 * lost bit). Measured on MI355X, join_type 2 against 0 on the same 2^20-row
 * build and 2^22-row all-hit probe page (profiles/outer_join_mark_cost.txt):
 * +0.026 ms on a 1.27 ms add_input (2 %) once the bits are set, +0.33 ms
 * (25 %) on a fresh bitmap, where the scattered matches of a random probe
 * order leave the wave combine nothing to merge. */
__global__ void k_mark_visited(const int32_t* __restrict__ ob, int64_t total,
                               uint64_t* __restrict__ visited)
{
    int lane = threadIdx.x % 64;
    int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t iw = i0 - lane; iw < total; iw += stride) {
        int64_t i = iw + lane;
        int32_t row = i < total ? ob[i] : -1;
        bool active = row >= 0;
        int64_t w = -1;
        uint64_t bit = 0;
        if (active) {
            w = row >> 6;
            bit = 1ull << (row & 63);
        }
        /* inclusive OR-scan over equal-w prefixes */
        #pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            uint64_t obit = __shfl_up(bit, off, 64);
            int64_t ow = __shfl_up(w, off, 64);
            if (lane >= off && ow == w) bit |= obit;
        }
        int64_t wnext = __shfl_down(w, 1, 64);
        bool last = active && (lane == 63 || wnext != w);
        if (last && (visited[w] & bit) != bit)
            atomicOr((unsigned long long*)&visited[w], (unsigned long long)bit);
    }
}

/* unvisited rows per bitmap word; the tail word is masked to n */
__global__ void k_unvisited_count(const uint64_t* __restrict__ visited, int64_t n,
                                  int32_t* __restrict__ counts)
{
    int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t words = (n + 63) / 64;
    for (; w < words; w += stride) {
        uint64_t mask = (w == words - 1 && (n & 63)) ? (1ull << (n & 63)) - 1 : ~0ull;
        counts[w] = __popcll(~visited[w] & mask);
    }
}

/* word w writes its unvisited rows, ascending, at offsets[w] */
__global__ void k_unvisited_rows(const uint64_t* __restrict__ visited, int64_t n,
                                 const int64_t* __restrict__ offsets,
                                 int32_t* __restrict__ rows)
{
    int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t words = (n + 63) / 64;
    for (; w < words; w += stride) {
        uint64_t mask = (w == words - 1 && (n & 63)) ? (1ull << (n & 63)) - 1 : ~0ull;
        uint64_t open = ~visited[w] & mask;
        int64_t at = offsets[w];
        while (open) {
            int b = __ffsll((unsigned long long)open) - 1;
            rows[at++] = (int32_t)(w * 64 + b);
            open &= open - 1;
        }
    }
}

/* ---- residual join filter (JoinFilterFunction: LookupJoinOperator tests it
 * on every position of the link chain before a pair counts as a match).
 * Every probe path ends in one probe-ordered candidate list (op, ob, n); the
 * kernels below turn it into the surviving list, so the step is as
 * path-independent as k_mark_visited, which then runs on the survivors.
 * All of them are elementwise over pairs or probe rows and separated by
 * launches; the scans between them are run_scan_counts. ---- */

/* one lane per candidate pair: keep[j] = the filter on (probe row op[j],
 * build row ob[j]) is non-NULL and non-zero (the filter operator's keep
 * rule). op is ascending, so probe cells load near-sequentially; build cells
 * are gathers. */
__global__ void k_pair_filter(const tg_expr_inst* __restrict__ prog, int count,
                              const KCol* __restrict__ pcols,
                              const KCol* __restrict__ bcols, int32_t n_probe,
                              const int32_t* __restrict__ op,
                              const int32_t* __restrict__ ob, int64_t n,
                              int32_t* __restrict__ keep)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; j < n; j += stride) {
        TVal v = eval_expr_cols(prog, count, PairCols{pcols, bcols, n_probe, op[j], ob[j]});
        keep[j] = (!v.null && tval_truthy(v)) ? 1 : 0;
    }
}

/* stable compaction by flag: kept pair j lands at at[j] + shift[op[j]]
 * (shift null: inner / right, where at = the exclusive scan of keep is the
 * whole position) */
__global__ void k_pair_place(const int32_t* __restrict__ keep,
                             const int64_t* __restrict__ at,
                             const int64_t* __restrict__ shift,
                             const int32_t* __restrict__ op,
                             const int32_t* __restrict__ ob, int64_t n,
                             int32_t* __restrict__ out_probe,
                             int32_t* __restrict__ out_build)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; j < n; j += stride) {
        if (!keep[j]) continue;
        int32_t i = op[j];
        int64_t pos = at[j] + (shift ? shift[i] : 0);
        out_probe[pos] = i;
        out_build[pos] = ob[j];
    }
}

/* survivors per probe row without an atomic: the candidates of probe row i
 * are one run of equal op, so with F = the exclusive scan of keep the row's
 * survivors are F[end] + keep[end] - F[start]. The run's first lane stores
 * the one, its last lane the other; rows without a candidate keep the zeros
 * both arrays were cleared to. (n <= INT32_MAX on this path, so F fits.) */
__global__ void k_pair_seg_bounds(const int32_t* __restrict__ op,
                                  const int32_t* __restrict__ keep,
                                  const int64_t* __restrict__ F, int64_t n,
                                  int32_t* __restrict__ seg_lo,
                                  int32_t* __restrict__ seg_hi)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; j < n; j += stride) {
        int32_t i = op[j];
        if (j == 0 || op[j - 1] != i) seg_lo[i] = (int32_t)F[j];
        if (j == n - 1 || op[j + 1] != i) seg_hi[i] = (int32_t)F[j] + keep[j];
    }
}

/* in place: seg_lo[i] -> surv[i], seg_hi[i] -> (surv[i] == 0) */
__global__ void k_pair_survivors(int32_t* __restrict__ seg_lo,
                                 int32_t* __restrict__ seg_hi, int64_t m)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < m; i += stride) {
        int32_t surv = seg_hi[i] - seg_lo[i];
        seg_lo[i] = surv;
        seg_hi[i] = surv == 0;
    }
}

/* probe-outer: the NULL-build row of survivor-less probe row i goes to
 * S[i] + Z[i] (kept pairs of earlier probe rows + NULL rows of earlier ones) */
__global__ void k_pair_null_rows(const int32_t* __restrict__ zero,
                                 const int64_t* __restrict__ S,
                                 const int64_t* __restrict__ Z, int64_t m,
                                 int32_t* __restrict__ out_probe,
                                 int32_t* __restrict__ out_build)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < m; i += stride) {
        if (!zero[i]) continue;
        int64_t pos = S[i] + Z[i];
        out_probe[pos] = (int32_t)i;
        out_build[pos] = -1;
    }
}

/* allocate and zero the bridge's visited bitmap on first need */
static tg_status bridge_ensure_visited(tg_join_bridge* b)
{
    if (b->visited) return TG_OK;
    int64_t words = (b->t.n + 63) / 64;
    if (words < 1) words = 1;
    TG_TRY(b->own.alloc(&b->visited, words * 8));
    TG_HIP_CHECK(hipMemsetAsync(b->visited, 0, words * 8, b->s->stream));
    return TG_OK;
}

__global__ void k_bitmap_concat(const uint64_t* __restrict__ src, int64_t n,
                                int64_t at, uint64_t* __restrict__ dst)
{
    /* dst preset to all-valid; clear dst bit (at+i) where src row i is null.
     * Works at any bit offset (the memcpy path needs 64-row alignment). */
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        if (!((src[i >> 6] >> (i & 63)) & 1)) {
            int64_t r = at + i;
            atomicAnd((unsigned long long*)&dst[r >> 6], ~(1ull << (r & 63)));
        }
    }
}

__global__ void k_off_rebase(const int32_t* __restrict__ src, int64_t n,
                             int32_t base, int32_t* __restrict__ dst)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = src[i] + base;
}

/* A/B on MI355X (Q3 SF100): CSR 98.0 ms/step vs open addressing 110.1 — CSR
 * default; TG_JOIN_CSR=0 selects the legacy path. Read once per process. */
static int join_use_csr()
{
    static int v = [] { const char* e = getenv("TG_JOIN_CSR"); return e ? atoi(e) : 1; }();
    return v;
}

/* ---- build operator ---- */
struct HashBuilderOp : tg_operator {
    tg_join_bridge* bridge = nullptr;
    bool set_only = false;          /* SetBuilderOperator: bitmap, no index */
    bool range_done_ = false;
    std::vector<int32_t> key_channels;
    std::vector<tg_type> types;
    std::vector<DevPage> pages;     /* PagesIndex */
    int64_t total_rows = 0;

    /* dynamic filter source: min/max and count of the non-null build keys */
    tg_status compute_key_range()
    {
        JoinTable& t = bridge->t;
        PoolScratch scratch(s);
        long long* d_mm = nullptr;
        TG_TRY(scratch.alloc(&d_mm, 3 * 8));
        long long init[3] = {INT64_MAX, INT64_MIN, 0};
        TG_HIP_CHECK(hipMemcpyAsync(d_mm, init, 24, hipMemcpyHostToDevice, s->stream));
        if (total_rows > 0) {
            hipLaunchKernelGGL(k_key_minmax, dim3(tg_grid_for(total_rows)), dim3(TG_BLOCK),
                               0, s->stream, t.keys, t.key_valid, total_rows,
                               d_mm, d_mm + 1, (unsigned long long*)(d_mm + 2));
            TG_HIP_CHECK(hipGetLastError());
        }
        long long mm[3];
        TG_HIP_CHECK(hipMemcpyAsync(mm, d_mm, 24, hipMemcpyDeviceToHost, s->stream));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        bridge->key_min = mm[0]; bridge->key_max = mm[1]; bridge->key_rows = mm[2];
        range_done_ = true;
        return TG_OK;
    }

    /* an all-valid bitmap over the build rows if any page carries one for
     * channel c, else *out stays null; owned by the bridge */
    tg_status alloc_valid(size_t c, uint64_t** out)
    {
        bool anynull = false;
        for (auto& p : pages)
            if (!p.blocks.empty() && p.blocks[c].valid) anynull = true;
        if (!anynull) return TG_OK;
        int64_t words = (total_rows + 63) / 64;
        TG_TRY(bridge->own.alloc(out, words * 8));
        TG_HIP_CHECK(hipMemsetAsync(*out, 0xFF, words * 8, s->stream));
        return TG_OK;
    }

    /* null bitmaps land at arbitrary bit offsets: k_bitmap_concat clears bit
     * (at + i) of dst per null row of the page block, whatever the page sizes */
    tg_status concat_valid(const DevBlock& pb, int64_t at, uint64_t* dst)
    {
        if (!pb.valid) return TG_OK;
        hipLaunchKernelGGL(k_bitmap_concat, dim3(tg_grid_for(pb.n)), dim3(TG_BLOCK),
                           0, s->stream, pb.valid, pb.n, at, dst);
        TG_HIP_CHECK(hipGetLastError());
        return TG_OK;
    }

    /* concatenate channel c across the accumulated pages, contiguous by
     * global build row. VARCHAR (PagesIndex keeps per-page
     * VariableWidthBlocks): each page's offsets are rebased onto a single
     * byte array, and a page's byte count is its last offset. */
    tg_status concat_channel(size_t c, DevBlock* b)
    {
        b->type = types[c];
        b->n = total_rows;
        const bool var = b->type == TG_VARCHAR;
        std::vector<int64_t> page_bytes(pages.size());
        int64_t total_bytes = 0;
        for (size_t pi = 0; pi < pages.size(); pi++) {
            const DevBlock& pb = pages[pi].blocks[c];
            int32_t tb = 0;
            if (var && pb.n) {
                TG_HIP_CHECK(hipMemcpy(&tb, pb.offsets + pb.n, 4,
                                       hipMemcpyDeviceToHost));
            }
            page_bytes[pi] = var ? tb : pb.n * b->elem_size();
            total_bytes += page_bytes[pi];
        }
        TG_TRY(bridge->own.alloc(&b->data, total_bytes));
        if (var) TG_TRY(bridge->own.alloc(&b->offsets, (total_rows + 1) * 4));
        TG_TRY(alloc_valid(c, &b->valid));
        int64_t at = 0, byte_at = 0;
        for (size_t pi = 0; pi < pages.size(); pi++) {
            const DevBlock& pb = pages[pi].blocks[c];
            if (page_bytes[pi]) {
                TG_HIP_CHECK(hipMemcpyAsync((char*)b->data + byte_at, pb.data,
                                            page_bytes[pi],
                                            hipMemcpyDeviceToDevice, s->stream));
            }
            if (var && pb.n) {
                hipLaunchKernelGGL(k_off_rebase, dim3(tg_grid_for(pb.n)),
                                   dim3(TG_BLOCK), 0, s->stream,
                                   pb.offsets, pb.n, (int32_t)byte_at,
                                   b->offsets + at);
                TG_HIP_CHECK(hipGetLastError());
            }
            TG_TRY(concat_valid(pb, at, b->valid));
            at += pb.n;
            byte_at += page_bytes[pi];
        }
        if (var) {
            int32_t tb32 = (int32_t)total_bytes;
            TG_HIP_CHECK(hipMemcpyAsync(b->offsets + total_rows, &tb32, 4,
                                        hipMemcpyHostToDevice, s->stream));
            TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        }
        return TG_OK;
    }

    /* the table arrays every build has: the flat key copy with its validity
     * bitmap, and for the legacy open-addressing table its slots and links */
    tg_status alloc_table()
    {
        JoinTable& t = bridge->t;
        if (!(join_use_csr() && total_rows > 0)) {
            TG_TRY(bridge->own.alloc(&t.slots, t.capacity * 4));
            TG_TRY(bridge->own.alloc(&t.links, total_rows * 4));
        }
        TG_TRY(bridge->own.alloc(&t.keys, total_rows * 8));
        return alloc_valid(key_channels[0], &t.key_valid);
    }

    /* single BIGINT key -> BigintPagesHash-style flat key copy; otherwise the
     * DefaultPagesHash-style generic channel compare (requires the CSR table;
     * the legacy open-addressing path stays single-key) */
    tg_status copy_keys()
    {
        JoinTable& t = bridge->t;
        t.generic = !(key_channels.size() == 1 &&
                      bridge->build_channels[key_channels[0]].type == TG_BIGINT);
        t.n_key_ch = (int32_t)key_channels.size();
        if (t.generic) {
            if (!join_use_csr()) { TG_SET_ERR("generic join keys require the CSR table"); return TG_ERR_UNSUPPORTED; }
            DevPage view;   /* non-owning view over the concatenated channels */
            view.n = total_rows;
            view.blocks = bridge->build_channels;
            tg_status st = make_kcols(s, view, key_channels.data(),
                                      (int)key_channels.size(), &bridge->d_bkeys);
            bridge->own.adopt(bridge->d_bkeys);
            t.bkeys = bridge->d_bkeys;
            return st;
        }
        const DevBlock& kb = bridge->build_channels[key_channels[0]];
        TG_HIP_CHECK(hipMemcpyAsync(t.keys, kb.data, total_rows * 8,
                                    hipMemcpyDeviceToDevice, s->stream));
        if (t.key_valid && kb.valid) {
            TG_HIP_CHECK(hipMemcpyAsync(t.key_valid, kb.valid,
                                        (total_rows + 63) / 64 * 8,
                                        hipMemcpyDeviceToDevice, s->stream));
        }
        return TG_OK;
    }

    /* dense-range key membership bitmap (single BIGINT key): the set
     * builder's whole table, or the dynamic-filter bitmap requested beside
     * the index. Best effort: a range beyond 2^33 leaves t.set_bitmap null. */
    tg_status build_key_bitmap()
    {
        JoinTable& t = bridge->t;
        TG_TRY(compute_key_range());
        int64_t range = bridge->key_rows > 0
                      ? bridge->key_max - bridge->key_min + 1 : 0;
        if (range <= 0 || range > (1ll << 33)) return TG_OK;   /* <= 1 GiB bitmap */
        int64_t words = (range + 63) / 64;
        uint64_t* bm = nullptr;
        TG_TRY(bridge->own.alloc(&bm, words * 8));
        TG_HIP_CHECK(hipMemsetAsync(bm, 0, words * 8, s->stream));
        hipLaunchKernelGGL(k_set_bits, dim3(tg_grid_for(total_rows)),
                           dim3(TG_BLOCK), 0, s->stream, t.keys,
                           t.key_valid, total_rows, bridge->key_min, bm);
        TG_HIP_CHECK(hipGetLastError());
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        t.set_bitmap = bm;
        t.set_min = bridge->key_min;
        t.set_max = bridge->key_max;
        return TG_OK;
    }

    /* CSR index: count -> region-local scan -> host scan of the region totals
     * -> scatter -> per-bucket sort; the temporaries end with this step */
    tg_status build_csr()
    {
        JoinTable& t = bridge->t;
        PoolScratch scratch(s);
        t.csr = 1;
        int64_t region_slots = t.capacity < JREG_SLOTS ? t.capacity : JREG_SLOTS;
        int64_t nreg = t.capacity / region_slots;
        TG_TRY(bridge->own.alloc(&t.bucket_off, (t.capacity + 1) * 4));
        TG_TRY(bridge->own.alloc(&t.csr_rows, total_rows * 4));
        uint32_t* d_slot_of = nullptr;
        int32_t* d_cnt = nullptr;       /* per-slot counts, then cursors */
        int32_t* d_rtotal = nullptr;
        int32_t* d_rbase = nullptr;
        TG_TRY(scratch.alloc(&d_slot_of, total_rows * 4));
        TG_TRY(scratch.alloc(&d_cnt, t.capacity * 4));
        TG_TRY(scratch.alloc(&d_rtotal, nreg * 4));
        TG_TRY(scratch.alloc(&d_rbase, nreg * 4));
        TG_HIP_CHECK(hipMemsetAsync(d_cnt, 0, t.capacity * 4, s->stream));
        hipLaunchKernelGGL(k_jc_count, dim3(tg_grid_for(total_rows)), dim3(TG_BLOCK),
                           0, s->stream, t, d_slot_of, d_cnt);
        TG_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_jc_local_off, dim3((uint32_t)nreg), dim3(TG_BLOCK),
                           0, s->stream, d_cnt, t.bucket_off, d_rtotal,
                           nreg, region_slots);
        TG_HIP_CHECK(hipGetLastError());
        std::vector<int32_t> rt(nreg), rb(nreg);
        TG_HIP_CHECK(hipMemcpyAsync(rt.data(), d_rtotal, nreg * 4,
                                    hipMemcpyDeviceToHost, s->stream));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        int32_t run = 0;
        for (int64_t r = 0; r < nreg; r++) { rb[r] = run; run += rt[r]; }
        int32_t total_indexed = run;    /* == total_rows minus null keys */
        t.has_null_key = (int64_t)total_indexed < total_rows ? 1 : 0;
        TG_HIP_CHECK(hipMemcpyAsync(d_rbase, rb.data(), nreg * 4,
                                    hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(k_jc_addbase, dim3(tg_grid_for(t.capacity)), dim3(TG_BLOCK),
                           0, s->stream, t.bucket_off, t.capacity, d_rbase,
                           region_slots);
        TG_HIP_CHECK(hipGetLastError());
        TG_HIP_CHECK(hipMemcpyAsync(t.bucket_off + t.capacity, &total_indexed, 4,
                                    hipMemcpyHostToDevice, s->stream));
        TG_HIP_CHECK(hipMemcpyAsync(d_cnt, t.bucket_off, t.capacity * 4,
                                    hipMemcpyDeviceToDevice, s->stream));
        hipLaunchKernelGGL(k_jc_scatter, dim3(tg_grid_for(total_rows)), dim3(TG_BLOCK),
                           0, s->stream, t, d_slot_of, d_cnt);
        TG_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_jc_sort, dim3(tg_grid_for(t.capacity)), dim3(TG_BLOCK),
                           0, s->stream, t);
        TG_HIP_CHECK(hipGetLastError());
        if (!t.generic) {
            TG_TRY(bridge->own.alloc(&t.csr_keys, total_rows * 8));
            hipLaunchKernelGGL(k_csr_keys, dim3(tg_grid_for(total_rows)),
                               dim3(TG_BLOCK), 0, s->stream, t, t.csr_keys);
            TG_HIP_CHECK(hipGetLastError());
        }
        /* A/B on MI355X (Q3 SF100): the 512 MB kv array RAISED probe
         * time (43.1 vs 39.7 ms per 10 launches) — the CSR arrays it
         * replaces are smaller and L2-cache better. Kept behind
         * TG_JOIN_KV=1 for small-table workloads. */
        static int use_kv = [] { const char* e = getenv("TG_JOIN_KV"); return e ? atoi(e) : 0; }();
        if (!t.generic && use_kv) {
            SlotKV* d_kv = nullptr;
            TG_TRY(bridge->own.alloc(&d_kv, t.capacity * (int64_t)sizeof(SlotKV)));
            hipLaunchKernelGGL(k_build_slotkv, dim3(tg_grid_for(t.capacity)),
                               dim3(TG_BLOCK), 0, s->stream, t, d_kv);
            TG_HIP_CHECK(hipGetLastError());
            t.kv = d_kv;
        }
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        return TG_OK;
    }

    /* legacy open-addressing table (TG_JOIN_CSR=0, and every empty build) */
    tg_status build_open_addressing()
    {
        JoinTable& t = bridge->t;
        hipLaunchKernelGGL(k_join_init, dim3(tg_grid_for(t.capacity)), dim3(TG_BLOCK),
                           0, s->stream, t.slots, t.capacity, t.links, total_rows);
        TG_HIP_CHECK(hipGetLastError());
        if (total_rows > 0) {
            hipLaunchKernelGGL(k_join_build, dim3(tg_grid_for(total_rows)), dim3(TG_BLOCK),
                               0, s->stream, t);
            TG_HIP_CHECK(hipGetLastError());
        }
        return TG_OK;
    }

    tg_status add_input(const tg_page* page) override
    {
        DevPage in;
        PageGuard gin(s, in);
        TG_TRY(tg_upload_page(s, page, &in));
        total_rows += in.n;
        pages.emplace_back(gin.take());
        return TG_OK;
    }

    tg_status finish() override
    {
        if (input_finished) return TG_OK;
        input_finished = true;
        JoinTable& t = bridge->t;
        t.n = total_rows;
        t.capacity = join_hash_size(total_rows);
        t.mask = t.capacity - 1;
        /* probe kernels encode a multi-match bucket slot as (int32_t)slot
         * (k_probe_count heads); a table beyond INT32_MAX slots would wrap
         * negative and be read back as a miss — reject at build, mirroring
         * BigintGroupByHash's own 2^30 capacity cap (BigintGroupByHash.java) */
        if (t.capacity > (int64_t)INT32_MAX) {
            TG_SET_ERR("join build of %lld rows needs %lld slots > INT32_MAX",
                       (long long)total_rows, (long long)t.capacity);
            return TG_ERR_OOM;
        }
        TG_TRY(alloc_table());
        bridge->build_channels.resize(types.size());
        for (size_t c = 0; c < types.size(); c++)
            TG_TRY(concat_channel(c, &bridge->build_channels[c]));
        TG_TRY(copy_keys());
        /* SetBuilderOperator path: the bitmap replaces the positional index
         * entirely (the 380M-row Q4 build spent ~63 ms in CSR construction a
         * semi join never needs). Beside a real index the bitmap is the
         * dynamic filter requested via tg_join_bridge_request_bitmap. */
        bool bitmap_built = false;
        if (!t.generic && total_rows > 0 && (set_only || bridge->want_bitmap)) {
            TG_TRY(build_key_bitmap());
            if (set_only && t.set_bitmap) {
                t.has_null_key = bridge->key_rows < total_rows ? 1 : 0;
                bitmap_built = true;
            }
        }
        if (!bitmap_built) {
            if (join_use_csr() && total_rows > 0) TG_TRY(build_csr());
            else TG_TRY(build_open_addressing());
        }
        /* dynamic filter source: min/max over non-null build keys
         * (single-BIGINT-key builds; generic keys report no range) */
        if (!t.generic && !range_done_) TG_TRY(compute_key_range());
        /* the legacy open-addressing build counts no indexed rows: take the
         * semi join's "build has a NULL key" from the non-null key count */
        if (!t.generic && !t.csr && !bitmap_built)
            t.has_null_key = bridge->key_rows < total_rows ? 1 : 0;
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        for (auto& p : pages) tg_free_page(s, &p);
        pages.clear();
        bridge->built = true;
        return TG_OK;
    }

    tg_status get_output(tg_page* out, int* finished) override
    {
        out->channel_count = 0;
        out->position_count = 0;
        out->blocks = nullptr;
        *finished = input_finished ? 1 : 0;
        return TG_OK;
    }

    ~HashBuilderOp() override
    {
        for (auto& p : pages) tg_free_page(s, &p);
    }
};

/* ---- probe operator ---- */
struct LookupJoinOp : tg_operator {
    tg_join_bridge* bridge = nullptr;
    std::vector<int32_t> key_channels;
    std::vector<tg_type> probe_types;
    std::vector<int32_t> probe_output;
    bool outer = false;             /* probe-outer (LEFT, FULL) */
    bool record = false;            /* build-outer (RIGHT, FULL): mark visited */
    bool counted = false;           /* still in bridge->recording */
    /* residual filter (tg_lookup_join_create_filtered): the compiled program
     * and the device array over ALL build channels live as long as the
     * operator; the array is made at the first add_input, when the bridge is
     * built */
    bool has_filter = false;
    ExprProgram filter{};
    int32_t n_probe_channels = 0;   /* TG_EXPR_COL indices below it name the probe page */
    KCol* d_bcols = nullptr;

    void release_recording()
    {
        if (counted) { bridge->recording--; counted = false; }
    }

    tg_status finish() override
    {
        release_recording();
        input_finished = true;
        return TG_OK;
    }

    /* Each probe path fills *d_op / *d_ob (probe row, build row per match,
     * owned by `out`) and *total; its own temporaries end with it, so they
     * are out of the pool's live set during the gathers. */

    /* partitioned single-pass probe + stable match sort */
    tg_status probe_partitioned(int64_t m, const ProbeKeys& pkc, int64_t tbl_bytes,
                                PoolScratch& out, int32_t** d_op, int32_t** d_ob,
                                int64_t* total)
    {
        const JoinTable& t = bridge->t;
        PoolScratch scratch(s);
        int64_t nparts = 1;
        while (tbl_bytes / nparts > (16ll << 20)) nparts <<= 1;
        if (nparts > t.capacity) nparts = t.capacity;
        int shift = 0;
        while (((int64_t)1 << shift) < t.capacity / nparts) shift++;
        uint32_t* d_slot_of = nullptr;
        int32_t* d_pc = nullptr;
        uint32_t* d_pi = nullptr;
        uint32_t* d_ps = nullptr;
        int64_t* d_pk = nullptr;
        unsigned long long* d_cnt = nullptr;
        TG_TRY(scratch.alloc(&d_slot_of, m * 4));
        TG_TRY(scratch.alloc(&d_pc, (nparts + 1) * 4));
        TG_TRY(scratch.alloc(&d_pi, m * 4));
        TG_TRY(scratch.alloc(&d_ps, m * 4));
        TG_TRY(scratch.alloc(&d_pk, m * 8));
        TG_TRY(scratch.alloc(&d_cnt, 8));
        TG_HIP_CHECK(hipMemsetAsync(d_pc, 0, (nparts + 1) * 4, s->stream));
        TG_HIP_CHECK(hipMemsetAsync(d_cnt, 0, 8, s->stream));
        hipLaunchKernelGGL(k_pb_slots, dim3(tg_grid_for(m)), dim3(TG_BLOCK),
                           (size_t)nparts * 4, s->stream, t, pkc, m, nparts,
                           shift, d_slot_of, d_pc);
        TG_HIP_CHECK(hipGetLastError());
        std::vector<int32_t> pc(nparts), pb(nparts);
        TG_HIP_CHECK(hipMemcpyAsync(pc.data(), d_pc, nparts * 4,
                                    hipMemcpyDeviceToHost, s->stream));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        int32_t run = 0;
        for (int64_t q = 0; q < nparts; q++) { pb[q] = run; run += pc[q]; }
        int64_t midx = run;               /* non-null probe rows */
        TG_HIP_CHECK(hipMemcpyAsync(d_pc, pb.data(), nparts * 4,
                                    hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(k_pb_scatter, dim3(2048), dim3(TG_BLOCK),
                           (size_t)nparts * 4, s->stream, t, pkc, m, shift,
                           d_slot_of, d_pc, nparts, d_pi, d_ps, d_pk);
        TG_HIP_CHECK(hipGetLastError());
        /* one k_pb_probe launch per non-empty partition, into lists of `cap` */
        auto probe_all = [&](int64_t cap) -> tg_status {
            for (int64_t q = 0; q < nparts; q++) {
                if (!pc[q]) continue;
                hipLaunchKernelGGL(k_pb_probe, dim3(1024), dim3(TG_BLOCK), 0, s->stream,
                                   t, (int64_t)pb[q], (int64_t)pb[q] + pc[q],
                                   d_pi, d_ps, d_pk, d_cnt, cap,
                                   (uint32_t*)*d_op, *d_ob);
                TG_HIP_CHECK(hipGetLastError());
            }
            return TG_OK;
        };
        /* first-try match cap (exact when build keys are unique, the
           usual case); k_pb_probe counts past it without writing, so an
           overflow is detected and retried with the exact size */
        int64_t cap = midx + t.n + 64;
        TG_TRY(out.alloc(d_op, cap * 4));
        TG_TRY(out.alloc(d_ob, cap * 4));
        TG_TRY(probe_all(cap));
        unsigned long long cnt = 0;
        TG_HIP_CHECK(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, s->stream));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        *total = (int64_t)cnt;
        TG_TRY(check_candidates(*total));
        if (*total > cap) {      /* many-to-many overflow: exact retry */
            out.release(*d_op);  /* back to the pool before the exact size is taken */
            out.release(*d_ob);
            cap = *total;
            TG_TRY(out.alloc(d_op, cap * 4));
            TG_TRY(out.alloc(d_ob, cap * 4));
            TG_HIP_CHECK(hipMemsetAsync(d_cnt, 0, 8, s->stream));
            TG_TRY(probe_all(cap));
            TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        }
        return run_sort_pairs_u32(s, (uint32_t*)*d_op, *d_ob, *total);
    }

    /* two-pass probe: count matches per probe row, scan, fill */
    tg_status probe_classic(int64_t m, const ProbeKeys& pkc, bool probe_outer,
                            PoolScratch& out, int32_t** d_op, int32_t** d_ob,
                            int64_t* total)
    {
        const JoinTable& t = bridge->t;
        PoolScratch scratch(s);
        int32_t* d_counts = nullptr;
        int32_t* d_heads = nullptr;
        int64_t* d_offsets = nullptr;
        int64_t* d_total = nullptr;
        TG_TRY(scratch.alloc(&d_counts, m * 4));
        TG_TRY(scratch.alloc(&d_heads, m * 4));
        TG_TRY(scratch.alloc(&d_offsets, m * 8));
        TG_TRY(scratch.alloc(&d_total, 8));
        hipLaunchKernelGGL(k_probe_count, dim3(tg_grid_for(m)), dim3(TG_BLOCK),
                           0, s->stream, t, pkc, m, probe_outer ? 1 : 0,
                           d_counts, d_heads);
        TG_HIP_CHECK(hipGetLastError());
        TG_TRY(run_scan_counts(s, d_counts, m, d_offsets, d_total));
        TG_HIP_CHECK(hipMemcpyAsync(total, d_total, 8, hipMemcpyDeviceToHost, s->stream));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        TG_TRY(check_candidates(*total));
        TG_TRY(out.alloc(d_op, *total * 4));
        TG_TRY(out.alloc(d_ob, *total * 4));
        hipLaunchKernelGGL(k_probe_fill, dim3(tg_grid_for(m)), dim3(TG_BLOCK),
                           0, s->stream, t, pkc, m, d_heads, d_offsets, *d_op, *d_ob);
        TG_HIP_CHECK(hipGetLastError());
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        return TG_OK;
    }

    /* the filtered path indexes its lists with int32 positions and hands the
     * total to the int32 gathers: say so instead of casting */
    tg_status check_candidates(int64_t total) const
    {
        if (has_filter && total > (int64_t)INT32_MAX) {
            TG_SET_ERR("filtered lookup join: %lld candidate pairs for one page exceed "
                       "INT32_MAX; probe with smaller pages", (long long)total);
            return TG_ERR_UNSUPPORTED;
        }
        return TG_OK;
    }

    /* host-side checks of the filter against this page and the built bridge,
     * before anything is uploaded or launched */
    tg_status check_filter_page(const tg_page* page) const
    {
        const int32_t n_build = (int32_t)bridge->build_types.size();
        for (int k = 0; k < filter.count; k++) {
            if (filter.insts[k].op != TG_EXPR_COL) continue;
            int32_t c = filter.insts[k].arg0;
            int32_t type;
            if (c >= 0 && c < n_probe_channels && c < page->channel_count)
                type = (int32_t)page->blocks[c].type;
            else if (c >= n_probe_channels && c - n_probe_channels < n_build)
                type = (int32_t)bridge->build_types[c - n_probe_channels];
            else {
                TG_SET_ERR("join filter column index %d outside the %d probe + %d build "
                           "channels (the page has %d)", c, n_probe_channels, n_build,
                           page->channel_count);
                return TG_ERR_INVALID_ARG;
            }
            if (type == TG_VARCHAR) {
                TG_SET_ERR("VARCHAR channel %d in a join filter", c);
                return TG_ERR_UNSUPPORTED;
            }
        }
        return TG_OK;
    }

    /* device KCol array over every channel of `blocks`; the caller owns it */
    tg_status upload_kcols(const std::vector<DevBlock>& blocks, KCol** d_out)
    {
        std::vector<KCol> cols(blocks.size());
        for (size_t c = 0; c < blocks.size(); c++)
            cols[c] = {blocks[c].data, blocks[c].valid, (int32_t)blocks[c].type, 0};
        size_t bytes = (cols.size() ? cols.size() : 1) * sizeof(KCol);
        TG_TRY(tg_pool_alloc(s, (void**)d_out, bytes));
        if (!cols.empty()) {
            TG_HIP_CHECK(hipMemcpyAsync(*d_out, cols.data(), cols.size() * sizeof(KCol),
                                        hipMemcpyHostToDevice, s->stream));
            TG_HIP_CHECK(hipStreamSynchronize(s->stream));   /* cols is a local */
        }
        return TG_OK;
    }

    /* The filter step: (d_op, d_ob, total) comes in as the inner candidate
     * list of the page, probe rows ascending, and leaves as the match list
     * the unfiltered operator would have produced had only the pairs that
     * pass the filter been equal: failing pairs removed, nothing else moved,
     * and under probe-outer one (i, -1) row for every probe row left without
     * a pair, at its place. With F, S, Z the exclusive scans of keep over
     * pairs, of survivors over probe rows and of (survivors == 0) over probe
     * rows: kept pair j -> F[j] + Z[op[j]], NULL row of i -> S[i] + Z[i]. */
    tg_status filter_matches(const DevPage& in, PoolScratch& out,
                             int32_t** d_op, int32_t** d_ob, int64_t* total)
    {
        const int64_t n = *total, m = in.n;
        if (n == 0 && !outer) return TG_OK;
        PoolScratch scratch(s);
        KCol* d_pcols = nullptr;
        TG_TRY(upload_kcols(in.blocks, &d_pcols));
        scratch.adopt(d_pcols);
        int32_t* d_keep = nullptr;
        int64_t* d_F = nullptr;
        int64_t* d_tot = nullptr;       /* kept pairs, NULL rows */
        TG_TRY(scratch.alloc(&d_keep, n * 4));
        TG_TRY(scratch.alloc(&d_F, n * 8));
        TG_TRY(scratch.alloc(&d_tot, 2 * 8));
        if (n > 0) {
            hipLaunchKernelGGL(k_pair_filter, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0,
                               s->stream, filter.d_insts, filter.count, d_pcols, d_bcols,
                               n_probe_channels, *d_op, *d_ob, n, d_keep);
            TG_HIP_CHECK(hipGetLastError());
        }
        TG_TRY(run_scan_counts(s, d_keep, n, d_F, d_tot));
        int32_t* d_surv = nullptr;      /* segment starts, then survivors per probe row */
        int32_t* d_zero = nullptr;      /* segment ends, then survivors == 0 */
        int64_t* d_S = nullptr;
        int64_t* d_Z = nullptr;
        if (outer) {
            TG_TRY(scratch.alloc(&d_surv, m * 4));
            TG_TRY(scratch.alloc(&d_zero, m * 4));
            TG_TRY(scratch.alloc(&d_S, m * 8));
            TG_TRY(scratch.alloc(&d_Z, m * 8));
            TG_HIP_CHECK(hipMemsetAsync(d_surv, 0, m * 4, s->stream));
            TG_HIP_CHECK(hipMemsetAsync(d_zero, 0, m * 4, s->stream));
            if (n > 0) {
                hipLaunchKernelGGL(k_pair_seg_bounds, dim3(tg_grid_for(n)), dim3(TG_BLOCK),
                                   0, s->stream, *d_op, d_keep, d_F, n, d_surv, d_zero);
                TG_HIP_CHECK(hipGetLastError());
            }
            hipLaunchKernelGGL(k_pair_survivors, dim3(tg_grid_for(m)), dim3(TG_BLOCK),
                               0, s->stream, d_surv, d_zero, m);
            TG_HIP_CHECK(hipGetLastError());
            TG_TRY(run_scan_counts(s, d_surv, m, d_S, d_tot));   /* same total again */
            TG_TRY(run_scan_counts(s, d_zero, m, d_Z, d_tot + 1));
        }
        int64_t tot[2] = {0, 0};
        TG_HIP_CHECK(hipMemcpyAsync(tot, d_tot, outer ? 16 : 8, hipMemcpyDeviceToHost,
                                    s->stream));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        const int64_t new_total = tot[0] + tot[1];
        if (new_total > (int64_t)INT32_MAX) {
            TG_SET_ERR("filtered lookup join: %lld output rows for one page exceed "
                       "INT32_MAX; probe with smaller pages", (long long)new_total);
            return TG_ERR_UNSUPPORTED;
        }
        int32_t* d_fp = nullptr;
        int32_t* d_fb = nullptr;
        TG_TRY(out.alloc(&d_fp, new_total * 4));
        TG_TRY(out.alloc(&d_fb, new_total * 4));
        if (n > 0 && tot[0] > 0) {
            hipLaunchKernelGGL(k_pair_place, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0,
                               s->stream, d_keep, d_F, d_Z, *d_op, *d_ob, n, d_fp, d_fb);
            TG_HIP_CHECK(hipGetLastError());
        }
        if (outer && tot[1] > 0) {
            hipLaunchKernelGGL(k_pair_null_rows, dim3(tg_grid_for(m)), dim3(TG_BLOCK), 0,
                               s->stream, d_zero, d_S, d_Z, m, d_fp, d_fb);
            TG_HIP_CHECK(hipGetLastError());
        }
        out.release(*d_op);     /* drains the stream: the candidates are done with */
        out.release(*d_ob);
        *d_op = d_fp;
        *d_ob = d_fb;
        *total = new_total;
        return TG_OK;
    }

    /* A/B on MI355X (Q3 SF100): partitioned probe 41 ms/step vs classic
     * 28.6 — the ~300 MB table already rides the 256 MB LLC, so the
     * extra partition passes (5.6 GB) and match sort never pay back.
     * Kept behind TG_JOIN_PART=1 for tables that outgrow the LLC. The
     * switches are read per call. */
    bool wants_partitioned(int64_t m, int64_t tbl_bytes) const
    {
        const JoinTable& t = bridge->t;
        const char* ep = getenv("TG_JOIN_PART");
        int use_part = ep ? atoi(ep) : 0;
        const char* emr = getenv("TG_JOIN_PART_MIN_ROWS");
        int64_t min_rows = emr ? atoll(emr) : (1 << 22);
        const char* emb = getenv("TG_JOIN_PART_MIN_BYTES");
        int64_t min_bytes = emb ? atoll(emb) : (64ll << 20);
        return use_part && !outer && t.csr && !t.generic && t.csr_keys &&
               m >= min_rows && tbl_bytes > min_bytes;
    }

    tg_status add_input(const tg_page* page) override
    {
        if (!bridge->built) { TG_SET_ERR("lookup source not built (finish the builder first)"); return TG_ERR_STATE; }
        if (bridge_is_set_only(bridge)) { TG_SET_ERR("set-builder bridge supports semi join only"); return TG_ERR_UNSUPPORTED; }
        TG_TRY(check_probe_keys(bridge, page, key_channels.data(), key_channels.size()));
        if (has_filter) {
            TG_TRY(check_filter_page(page));
            if (!d_bcols) TG_TRY(upload_kcols(bridge->build_channels, &d_bcols));
        }
        if (!record) bridge->plain_probed = true;
        DevPage in, outp;
        PageGuard gin(s, in), gout(s, outp);
        PoolScratch scratch(s);          /* after the pages: destroyed, and drained, first */
        TG_TRY(tg_upload_page(s, page, &in));
        const JoinTable& t = bridge->t;
        ProbeKeys pkc{};
        TG_TRY(probe_keys_of(s, t, in, key_channels.data(), (int)key_channels.size(),
                             scratch, &pkc));
        int32_t* d_op = nullptr;
        int32_t* d_ob = nullptr;
        int64_t total = 0;
        int64_t tbl_bytes = t.capacity * 4 + t.n * 12;
        if (wants_partitioned(in.n, tbl_bytes))
            TG_TRY(probe_partitioned(in.n, pkc, tbl_bytes, scratch, &d_op, &d_ob, &total));
        else   /* with a filter the probe is inner: filter_matches adds the NULL rows */
            TG_TRY(probe_classic(in.n, pkc, outer && !has_filter, scratch,
                                 &d_op, &d_ob, &total));
        if (has_filter)
            TG_TRY(filter_matches(in, scratch, &d_op, &d_ob, &total));

        /* build-outer: whichever path ran, d_ob[0..total) is the matched
         * build row list (after the filter: the surviving pairs only) — record it (stream-ordered before the gathers) */
        if (record) {
            TG_TRY(bridge_ensure_visited(bridge));
            if (total > 0) {
                hipLaunchKernelGGL(k_mark_visited, dim3(tg_grid_for(total)), dim3(TG_BLOCK),
                                   0, s->stream, d_ob, total, bridge->visited);
                TG_HIP_CHECK(hipGetLastError());
            }
        }

        /* output: probe output channels gathered by probe row, then build
         * output channels gathered by build row (LookupJoinPageBuilder) */
        outp.n = total;
        for (int32_t ch : probe_output) {
            outp.blocks.emplace_back();
            TG_TRY(run_gather(s, in.blocks[ch], d_op, (int32_t)total, &outp.blocks.back()));
        }
        for (int32_t ch : bridge->build_output_channels) {
            outp.blocks.emplace_back();
            TG_TRY(run_gather(s, bridge->build_channels[ch], d_ob, (int32_t)total,
                              &outp.blocks.back(), outer /* -1 positions become NULL */));
        }
        stage_output(gout.take());
        return TG_OK;
    }

    tg_status get_output(tg_page* out, int* finished) override
    {
        emit_staged(out, finished);
        return TG_OK;
    }

    ~LookupJoinOp() override
    {
        release_recording();     /* closed unfinished: the bridge outlives us */
        if (has_filter) tg_free_expr(s, &filter);
        if (d_bcols) tg_pool_free(s, d_bcols);
        for (auto& p : out_pages_) tg_free_page(s, &p);
    }
};

/* ---- lookup-outer operator (LookupOuterOperator.java): a source operator
 * that emits, once every recording probe operator on the bridge has
 * finished, one row per build row no probe row matched — the probe output
 * channels all NULL, then the build output channels gathered from the build
 * row; ascending global build row order, one page ---- */
struct LookupOuterOp : tg_operator {
    tg_join_bridge* bridge = nullptr;
    std::vector<tg_type> probe_out_types;
    bool emitted = false;

    int needs_input() override { return 0; }

    tg_status add_input(const tg_page*) override
    {
        TG_SET_ERR("the lookup-outer operator is a source: it takes no input");
        return TG_ERR_STATE;
    }

    /* an all-NULL column: cleared validity bits, zeroed data, VARCHAR cells
     * of zero length (the LEFT join's build-side convention) */
    tg_status null_column(tg_type type, int64_t count, DevBlock* b)
    {
        b->type = type;
        b->n = count;
        int64_t words = (count + 63) / 64;
        TG_POOL_ALLOC(s, &b->valid, words * 8);
        TG_HIP_CHECK(hipMemsetAsync(b->valid, 0, words * 8, s->stream));
        if (type == TG_VARCHAR) {
            TG_POOL_ALLOC(s, &b->offsets, (count + 1) * 4);
            TG_HIP_CHECK(hipMemsetAsync(b->offsets, 0, (count + 1) * 4, s->stream));
            TG_POOL_ALLOC(s, &b->data, 1);
            return TG_OK;
        }
        TG_POOL_ALLOC(s, &b->data, count * b->elem_size());
        TG_HIP_CHECK(hipMemsetAsync(b->data, 0, count * b->elem_size(), s->stream));
        return TG_OK;
    }

    tg_status emit_unmatched()
    {
        const int64_t n = bridge->t.n;
        if (n == 0) return TG_OK;
        /* no recording operator ever added a page: every row is unvisited */
        TG_TRY(bridge_ensure_visited(bridge));
        DevPage outp;
        PageGuard gout(s, outp);
        PoolScratch scratch(s);
        int64_t words = (n + 63) / 64;
        int32_t* d_counts = nullptr;
        int64_t* d_offsets = nullptr;
        int64_t* d_total = nullptr;
        TG_TRY(scratch.alloc(&d_counts, words * 4));
        TG_TRY(scratch.alloc(&d_offsets, words * 8));
        TG_TRY(scratch.alloc(&d_total, 8));
        hipLaunchKernelGGL(k_unvisited_count, dim3(tg_grid_for(words)), dim3(TG_BLOCK),
                           0, s->stream, bridge->visited, n, d_counts);
        TG_HIP_CHECK(hipGetLastError());
        TG_TRY(run_scan_counts(s, d_counts, words, d_offsets, d_total));
        int64_t total = 0;
        TG_HIP_CHECK(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, s->stream));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        if (total == 0) return TG_OK;
        int32_t* d_rows = nullptr;
        TG_TRY(scratch.alloc(&d_rows, total * 4));
        hipLaunchKernelGGL(k_unvisited_rows, dim3(tg_grid_for(words)), dim3(TG_BLOCK),
                           0, s->stream, bridge->visited, n, d_offsets, d_rows);
        TG_HIP_CHECK(hipGetLastError());
        outp.n = total;
        for (tg_type ty : probe_out_types) {
            outp.blocks.emplace_back();
            TG_TRY(null_column(ty, total, &outp.blocks.back()));
        }
        for (int32_t ch : bridge->build_output_channels) {
            outp.blocks.emplace_back();
            TG_TRY(run_gather(s, bridge->build_channels[ch], d_rows, (int32_t)total,
                              &outp.blocks.back()));
        }
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        stage_output(gout.take());
        return TG_OK;
    }

    tg_status get_output(tg_page* out, int* finished) override
    {
        if (!emitted) {
            /* all state rules are checked here, on the host, before a launch */
            if (!bridge->built) { TG_SET_ERR("lookup source not built (finish the builder first)"); return TG_ERR_STATE; }
            if (bridge_is_set_only(bridge)) { TG_SET_ERR("set-builder bridge supports semi join only"); return TG_ERR_UNSUPPORTED; }
            if (bridge->recording > 0) {
                TG_SET_ERR("%d recording lookup join operator(s) on this bridge have not finished",
                           bridge->recording);
                return TG_ERR_STATE;
            }
            if (bridge->plain_probed) {
                TG_SET_ERR("a join_type 0 or 1 lookup join probed this bridge: its matches were not recorded");
                return TG_ERR_STATE;
            }
            TG_TRY(emit_unmatched());
            emitted = true;
            input_finished = true;
        }
        emit_staged(out, finished);
        return TG_OK;
    }

    ~LookupOuterOp() override
    {
        for (auto& p : out_pages_) tg_free_page(s, &p);
    }
};

extern "C" tg_status tg_join_bridge_create(tg_session* s, tg_join_bridge** out)
{
    if (!s || !out) { TG_SET_ERR("null arg"); return TG_ERR_INVALID_ARG; }
    *out = new tg_join_bridge(s);
    return TG_OK;
}

/* the bridge's owner drains the stream and frees every table buffer */
extern "C" void tg_join_bridge_close(tg_join_bridge* b)
{
    delete b;
}

extern "C" tg_status tg_hash_builder_create(tg_session* s, tg_join_bridge* bridge,
    const int32_t* build_types, int32_t n_build_channels,
    const int32_t* key_channels, int32_t n_key_channels,
    const int32_t* output_channels, int32_t n_output_channels,
    tg_operator** out)
{
    if (!s || !bridge || !build_types || !key_channels || n_key_channels < 1 ||
        n_key_channels > 7) {
        TG_SET_ERR("1..7 join key channels");
        return TG_ERR_INVALID_ARG;
    }
    auto* op = new HashBuilderOp();
    op->s = s;
    op->bridge = bridge;
    op->key_channels.assign(key_channels, key_channels + n_key_channels);
    for (int i = 0; i < n_build_channels; i++)
        op->types.push_back((tg_type)build_types[i]);
    bridge->build_types = op->types;
    bridge->key_channels = op->key_channels;
    bridge->build_output_channels.assign(output_channels, output_channels + n_output_channels);
    *out = op;
    return TG_OK;
}

/* SetBuilderOperator analog (semi-join source: ChannelSet membership only;
 * dense key ranges use a bitmap, sparse ranges fall back to the CSR index) */
extern "C" tg_status tg_set_builder_create(tg_session* s, tg_join_bridge* bridge,
    const int32_t* build_types, int32_t n_build_channels,
    int32_t key_channel, tg_operator** out)
{
    int32_t kc = key_channel;
    TG_TRY(tg_hash_builder_create(s, bridge, build_types, n_build_channels,
                                  &kc, 1, nullptr, 0, out));
    static_cast<HashBuilderOp*>(*out)->set_only = true;
    return TG_OK;
}

/* ---- semi join (operator/HashSemiJoinOperator.java: appends a BOOLEAN
 * "matched" channel to the probe page; null probe keys yield NULL) ---- */
__global__ void k_semi_probe(JoinTable t, ProbeKeys p, int64_t m,
                             int8_t* __restrict__ match, uint64_t* __restrict__ mvalid)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < m; i += stride) {
        /* three-valued IN semantics (HashSemiJoinOperator.java:180-201):
         * probe null -> false if the build set is empty, else NULL;
         * miss against a set containing NULL -> NULL. */
        if (t.n == 0) {      /* empty build: false and valid, NULL probes too */
            match[i] = 0;
            continue;
        }
        if (probe_null(t, p, i)) {
            match[i] = 0;
            atomicAnd((unsigned long long*)&mvalid[i >> 6], ~(1ull << (i & 63)));
            continue;
        }
        int8_t hit = 0;
        if (t.set_bitmap) {
            int64_t pk = p.pk[i];
            if (pk >= t.set_min && pk <= t.set_max) {
                uint64_t k = (uint64_t)(pk - t.set_min);
                hit = (t.set_bitmap[k >> 6] >> (k & 63)) & 1 ? 1 : 0;
            }
            match[i] = hit;
            if (!hit && t.has_null_key)
                atomicAnd((unsigned long long*)&mvalid[i >> 6], ~(1ull << (i & 63)));
            continue;
        }
        int64_t slot = (int64_t)probe_slot(t, p, i);
        if (t.kv) {
            SlotKV e = t.kv[slot];
            if (e.row >= 0) hit = (e.key == p.pk[i]);
            else if (e.row == -2) {
                for (int32_t x = t.bucket_off[slot]; x < t.bucket_off[slot + 1] && !hit; x++)
                    hit = probe_matches(t, p, i, t.csr_rows[x]);
            }
        }
        else if (t.csr && t.csr_keys) {
            int64_t key = p.pk[i];
            for (int32_t x = t.bucket_off[slot]; x < t.bucket_off[slot + 1] && !hit; x++)
                hit = (t.csr_keys[x] == key);
        }
        else if (t.csr) {
            for (int32_t x = t.bucket_off[slot]; x < t.bucket_off[slot + 1] && !hit; x++)
                hit = probe_matches(t, p, i, t.csr_rows[x]);
        }
        else {
            int64_t key = p.pk[i];
            int32_t cur;
            while ((cur = t.slots[slot]) != -1) {
                if (t.keys[cur] == key) { hit = 1; break; }
                slot = (slot + 1) & t.mask;
            }
        }
        match[i] = hit;
        if (!hit && t.has_null_key)
            atomicAnd((unsigned long long*)&mvalid[i >> 6], ~(1ull << (i & 63)));
    }
}

struct SemiJoinOp : tg_operator {
    tg_join_bridge* bridge = nullptr;
    int32_t key_channel = 0;

    tg_status add_input(const tg_page* page) override
    {
        if (!bridge->built) { TG_SET_ERR("lookup source not built"); return TG_ERR_STATE; }
        /* the probe context below carries ONE key channel, while the kernels
         * loop to the build's channel count */
        if (bridge->key_channels.size() != 1) {
            TG_SET_ERR("semi join takes a single key channel; the build has %zu",
                       bridge->key_channels.size());
            return TG_ERR_UNSUPPORTED;
        }
        TG_TRY(check_probe_keys(bridge, page, &key_channel, 1));
        DevPage in;
        PageGuard gin(s, in);
        PoolScratch scratch(s);
        TG_TRY(tg_upload_page(s, page, &in));
        ProbeKeys pkc{};
        TG_TRY(probe_keys_of(s, bridge->t, in, &key_channel, 1, scratch, &pkc));
        /* the match channel is appended to the guarded probe page, which then
         * moves into the output whole: its blocks and the match */
        in.blocks.emplace_back();
        DevBlock& mb = in.blocks.back();
        mb.type = TG_BOOLEAN;
        mb.n = in.n;
        TG_POOL_ALLOC(s, &mb.data, in.n ? in.n : 1);
        int64_t words = (in.n + 63) / 64;
        TG_POOL_ALLOC(s, &mb.valid, (words ? words : 1) * 8);
        TG_HIP_CHECK(hipMemsetAsync(mb.valid, 0xFF, words * 8, s->stream));
        hipLaunchKernelGGL(k_semi_probe, dim3(tg_grid_for(in.n)), dim3(TG_BLOCK),
                           0, s->stream, bridge->t, pkc, in.n, (int8_t*)mb.data, mb.valid);
        TG_HIP_CHECK(hipGetLastError());
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        stage_output(gin.take());
        return TG_OK;
    }

    tg_status get_output(tg_page* out, int* finished) override
    {
        emit_staged(out, finished);
        return TG_OK;
    }

    ~SemiJoinOp() override
    {
        for (auto& p : out_pages_) tg_free_page(s, &p);
    }
};

extern "C" tg_status tg_semi_join_create(tg_session* s, tg_join_bridge* bridge,
                                         int32_t key_channel, tg_operator** out)
{
    if (!s || !bridge || !out) { TG_SET_ERR("null arg"); return TG_ERR_INVALID_ARG; }
    auto* op = new SemiJoinOp();
    op->s = s;
    op->bridge = bridge;
    op->key_channel = key_channel;
    *out = op;
    return TG_OK;
}

extern "C" tg_status tg_lookup_join_create(tg_session* s, tg_join_bridge* bridge,
    const int32_t* probe_types, int32_t n_probe_channels,
    const int32_t* key_channels, int32_t n_key_channels,
    const int32_t* probe_output_channels, int32_t n_probe_output,
    tg_operator** out)
{
    if (!s || !bridge || !key_channels || n_key_channels < 1 || n_key_channels > 7) {
        TG_SET_ERR("1..7 join key channels");
        return TG_ERR_INVALID_ARG;
    }
    auto* op = new LookupJoinOp();
    op->s = s;
    op->bridge = bridge;
    op->key_channels.assign(key_channels, key_channels + n_key_channels);
    for (int i = 0; i < n_probe_channels; i++)
        op->probe_types.push_back((tg_type)probe_types[i]);
    op->probe_output.assign(probe_output_channels, probe_output_channels + n_probe_output);
    *out = op;
    return TG_OK;
}

extern "C" tg_status tg_lookup_join_create_ex(tg_session* s, tg_join_bridge* bridge,
    const int32_t* probe_types, int32_t n_probe_channels,
    const int32_t* key_channels, int32_t n_key_channels,
    const int32_t* probe_output_channels, int32_t n_probe_output,
    int32_t join_type, tg_operator** out)
{
    if (join_type < 0 || join_type > 3) {
        TG_SET_ERR("join_type %d: 0 inner, 1 probe-outer, 2 build-outer, 3 full", join_type);
        return TG_ERR_INVALID_ARG;
    }
    TG_TRY(tg_lookup_join_create(s, bridge, probe_types, n_probe_channels,
                                 key_channels, n_key_channels,
                                 probe_output_channels, n_probe_output, out));
    auto* op = static_cast<LookupJoinOp*>(*out);
    op->outer = (join_type == 1 || join_type == 3);
    if (join_type >= 2) {    /* build-outer: counted until finished or closed */
        op->record = true;
        op->counted = true;
        bridge->recording++;
    }
    return TG_OK;
}

/* tg_lookup_join_create_ex with a residual filter on the join condition */
extern "C" tg_status tg_lookup_join_create_filtered(tg_session* s, tg_join_bridge* bridge,
    const int32_t* probe_types, int32_t n_probe_channels,
    const int32_t* key_channels, int32_t n_key_channels,
    const int32_t* probe_output_channels, int32_t n_probe_output,
    int32_t join_type, const tg_expr* filter, tg_operator** out)
{
    if (filter) {
        if (n_probe_channels < 0) { TG_SET_ERR("n_probe_channels %d", n_probe_channels); return TG_ERR_INVALID_ARG; }
        TG_TRY(check_expr_depth(filter, TG_ERR_INVALID_ARG));
    }
    TG_TRY(tg_lookup_join_create_ex(s, bridge, probe_types, n_probe_channels,
                                    key_channels, n_key_channels,
                                    probe_output_channels, n_probe_output,
                                    join_type, out));
    if (!filter) return TG_OK;
    auto* op = static_cast<LookupJoinOp*>(*out);
    tg_status st = tg_compile_expr(s, filter, &op->filter);
    op->has_filter = true;       /* the destructor frees whatever was compiled */
    op->n_probe_channels = n_probe_channels;
    if (st != TG_OK) { delete op; *out = nullptr; return st; }
    return TG_OK;
}

extern "C" tg_status tg_lookup_outer_create(tg_session* s, tg_join_bridge* bridge,
    const int32_t* probe_output_types, int32_t n_probe_output, tg_operator** out)
{
    if (!s || !bridge || !out || n_probe_output < 0 ||
        (n_probe_output > 0 && !probe_output_types)) {
        TG_SET_ERR("null arg");
        return TG_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n_probe_output; i++) {
        if (probe_output_types[i] < TG_BIGINT || probe_output_types[i] > TG_VARCHAR) {
            TG_SET_ERR("probe output type %d at position %d", probe_output_types[i], i);
            return TG_ERR_INVALID_ARG;
        }
    }
    auto* op = new LookupOuterOp();
    op->s = s;
    op->bridge = bridge;
    for (int i = 0; i < n_probe_output; i++)
        op->probe_out_types.push_back((tg_type)probe_output_types[i]);
    *out = op;
    return TG_OK;
}

/* dynamic filter: the build side's non-null key range (valid after the
 * builder's finish); has_rows=0 means the probe side can skip entirely */
extern "C" tg_status tg_join_bridge_key_range(tg_join_bridge* b, int64_t* key_min,
                                              int64_t* key_max, int64_t* key_rows)
{
    if (!b || !b->built) { TG_SET_ERR("lookup source not built"); return TG_ERR_STATE; }
    if (b->t.generic) { TG_SET_ERR("key range is tracked for single BIGINT keys"); return TG_ERR_UNSUPPORTED; }
    if (key_min) *key_min = b->key_min;
    if (key_max) *key_max = b->key_max;
    if (key_rows) *key_rows = b->key_rows;
    return TG_OK;
}

/* request a probe-side dynamic-filter bitmap from this bridge's build
 * (must be called before the builder's finish) */
extern "C" tg_status tg_join_bridge_request_bitmap(tg_join_bridge* b)
{
    if (!b) { TG_SET_ERR("null bridge"); return TG_ERR_INVALID_ARG; }
    b->want_bitmap = true;
    return TG_OK;
}

/* internal: fetch the bitmap for the filter operator (ops_filter.hip) */
bool tg_bridge_df(tg_join_bridge* b, const uint64_t** bm, int64_t* mn, int64_t* mx)
{
    if (!b || !b->built || !b->t.set_bitmap) return false;
    *bm = b->t.set_bitmap;
    *mn = b->t.set_min;
    *mx = b->t.set_max;
    return true;
}
