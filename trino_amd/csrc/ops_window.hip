/* ops_window.hip — Window operator (operator/WindowOperator.java analog).
 *
 * Accumulates input pages like TopN; at finish it sorts every row on the
 * device by (partition channels ASC NULLS LAST, sort channels), marks the
 * partition and peer-group starts, and computes every window function as a
 * SEGMENTED SCAN of i64 values plus, for the RANGE and whole-partition
 * frames, a gather through the index of the segment's last row. One output
 * page: the input channels in sorted order, then one BIGINT channel per spec.
 *
 * The segmented scan is the hot path. It is an inclusive scan
 * under the associative pair operator
 *     (f1,v1) (+) (f2,v2) = (f1|f2, f2 ? v2 : op(v1,v2))
 * with op one of + / min / max on i64, built like run_scan_i32 as three
 * launches: a wave per WSCAN_CHUNK rows reduces its chunk to one carry pair,
 * the carries are scanned by the same operator (one wave up to
 * WSCAN_ONE_WAVE entries, recursion above), and the same chunk pass runs
 * again with each chunk's incoming carry. No block waits on another block:
 * no look-back, no flag polling, no atomics, no fences; integer + / min / max
 * give the same bits under any association, so the result is bit-exact.
 *
 * On top of that sits the frame layer of tg_window_create_ex:
 * every frame becomes an index range [lo, hi] per row (k_win_bounds); counts
 * and sums over ROWS BETWEEN are differences of the partition-headed scans
 * (k_win_frame_emit), min / max over a frame open at one end is a forward or
 * reverse scan read at the other end, min / max over a frame bounded at both
 * ends is a sparse table evaluated level by level (k_win_level), and lag /
 * lead / first_value / last_value / nth_value are one gather of the sorted
 * payload cells (k_win_value). The output channel of a value function has its
 * input channel's type.
 *
 * The TopNRanking operator (ranking <= N per partition) follows
 * the Window at the end of the file and shares its boundary kernel and scan.
 */
#include "sort_keys.h"
#include "operators.h"
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <tuple>

#define WSCAN_CHUNK 1024
#define WSCAN_ONE_WAVE 1024
#define WSCAN_BATCH 4      /* 64-row groups loaded ahead of their scan */

enum { WOP_ADD = 0, WOP_MIN = 1, WOP_MAX = 2 };
/* where the scanned value of a position comes from */
enum {
    WSRC_ARRAY = 0,    /* vals[i] */
    WSRC_ONE = 1,      /* 1 */
    WSRC_INDEX = 2,    /* i */
    WSRC_FLAG = 3,     /* (flags[i] & val_mask) ? 1 : 0 */
    WSRC_MASKED = 4,   /* (flags[i] & val_mask) ? vals[i] : 0 */
    WSRC_NEUTRAL = 5   /* aux[i] ? vals[i] : identity(op)   (NULL-neutralised) */
};
enum { WFLAG_PARTITION = 1, WFLAG_PEER = 2 };

/* one scan's input. A head flag is (flags[i] & head_mask) != 0; position 0 is
 * always a head. `reverse` scans from the last row towards the first with a
 * head wherever the forward segmentation ENDS (the next row is a head), which
 * turns a max scan of WSRC_INDEX into "index of my segment's last row". */
struct WscanIn {
    const int64_t* vals;
    const int64_t* aux;
    const uint8_t* flags;
    int64_t n;
    int32_t head_mask, val_mask, src, op, reverse;
};

__device__ static inline int64_t wscan_identity(int32_t op)
{
    return op == WOP_ADD ? 0 : op == WOP_MIN ? INT64_MAX : INT64_MIN;
}

__device__ static inline int64_t wscan_op(int32_t op, int64_t a, int64_t b)
{
    if (op == WOP_ADD) return (int64_t)((uint64_t)a + (uint64_t)b);   /* wraps */
    if (op == WOP_MIN) return a < b ? a : b;
    return a > b ? a : b;
}

/* physical index of logical scan position p */
__device__ static inline int64_t wscan_phys(const WscanIn& in, int64_t p)
{
    return in.reverse ? in.n - 1 - p : p;
}

__device__ static inline void wscan_load(const WscanIn& in, int64_t p, int& f, int64_t& v)
{
    int64_t i = wscan_phys(in, p);
    int fl = in.flags[i];
    if (in.reverse) f = (i == in.n - 1) || (in.flags[i + 1] & in.head_mask);
    else f = (i == 0) || (fl & in.head_mask);
    switch (in.src) {
        case WSRC_ARRAY: v = in.vals[i]; break;
        case WSRC_ONE: v = 1; break;
        case WSRC_INDEX: v = i; break;
        case WSRC_FLAG: v = (fl & in.val_mask) ? 1 : 0; break;
        case WSRC_MASKED: v = (fl & in.val_mask) ? in.vals[i] : 0; break;
        default: v = in.aux[i] ? in.vals[i] : wscan_identity(in.op); break;
    }
}

/* the chunk pass: one wave walks logical positions [lo, hi) in 64-row groups.
 * Inside a group the pair operator runs as six __shfl_up steps on the values
 * alone. The flag half of the pair needs no shuffle: one __ballot gives every
 * lane the group's heads, hence `start`, the lane of the nearest head at or
 * before it (-1: none), and "no head between the two lanes" (f2 == 0 of the
 * pair being appended) is `lane - off >= start`. A lane whose partner lies
 * before its head already holds its whole segment. (rf, rv) is the running
 * pair carried from group to group (and, in the apply launch, into the chunk
 * from the scanned carries); it reaches exactly the lanes with start < 0.
 * lo and hi are wave-uniform, so every lane takes every shuffle. Lanes past
 * hi hold (0, identity) and so copy their left neighbour: lane 63 always
 * ends with the group's total. */
template <bool WRITE>
__device__ static inline void wscan_chunk(const WscanIn& in, int64_t lo, int64_t hi,
                                          int lane, int& rf, int64_t& rv, int64_t* out)
{
    const int32_t op = in.op;
    /* WSCAN_BATCH groups are loaded before the first of them is scanned, so
     * a wave keeps that many loads in flight instead of paying one memory
     * round trip per group; a group wholly past hi is (0, identity) in every
     * lane and passes the running pair through unchanged */
    for (int64_t g = lo; g < hi; g += 64 * WSCAN_BATCH) {
        int fs[WSCAN_BATCH];
        int64_t vs[WSCAN_BATCH];
        #pragma unroll
        for (int k = 0; k < WSCAN_BATCH; k++) {
            int64_t p = g + 64 * k + lane;
            fs[k] = 0;
            vs[k] = wscan_identity(op);
            if (p < hi) wscan_load(in, p, fs[k], vs[k]);
        }
        #pragma unroll
        for (int k = 0; k < WSCAN_BATCH; k++) {
            int64_t p = g + 64 * k + lane;
            int64_t v = vs[k];
            uint64_t heads = __ballot(fs[k]);
            uint64_t mine = heads & (~0ull >> (63 - lane));     /* heads in lanes 0..lane */
            int start = mine ? 63 - __clzll((long long)mine) : -1;
            #pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                int64_t ov = (int64_t)__shfl_up((long long)v, off, 64);
                if (lane >= off && lane - off >= start) v = wscan_op(op, ov, v);
            }
            if (start < 0) v = wscan_op(op, rv, v);
            if (WRITE && p < hi) out[wscan_phys(in, p)] = v;
            rv = (int64_t)__shfl((long long)v, 63, 64);
            rf |= heads != 0;
        }
    }
}

/* launch 1: chunk c -> carry pair (carry_f[c], carry_v[c]) */
__global__ void k_wscan_reduce(WscanIn in, int64_t nchunks,
                               uint8_t* __restrict__ carry_f, int64_t* __restrict__ carry_v)
{
    int64_t c = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (c >= nchunks) return;
    int lane = threadIdx.x % 64;
    int64_t lo = c * WSCAN_CHUNK, hi = min(lo + (int64_t)WSCAN_CHUNK, in.n);
    int rf = 0;
    int64_t rv = wscan_identity(in.op);
    wscan_chunk<false>(in, lo, hi, lane, rf, rv, nullptr);
    if (lane == 0) {
        carry_f[c] = rf ? 1 : 0;
        carry_v[c] = rv;
    }
}

/* launch 3: the chunk pass again, starting from the inclusive scan of the
 * carries before chunk c */
__global__ void k_wscan_apply(WscanIn in, int64_t nchunks,
                              const int64_t* __restrict__ carry_scanned, int64_t* out)
{
    int64_t c = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (c >= nchunks) return;
    int lane = threadIdx.x % 64;
    int64_t lo = c * WSCAN_CHUNK, hi = min(lo + (int64_t)WSCAN_CHUNK, in.n);
    int rf = 0;
    int64_t rv = c ? carry_scanned[c - 1] : wscan_identity(in.op);
    wscan_chunk<true>(in, lo, hi, lane, rf, rv, out);
}

/* the whole input by one wave (n <= WSCAN_ONE_WAVE) */
__global__ void k_wscan_one_wave(WscanIn in, int64_t* out)
{
    if (blockIdx.x || threadIdx.x >= 64) return;
    int rf = 0;
    int64_t rv = wscan_identity(in.op);
    wscan_chunk<true>(in, 0, in.n, threadIdx.x, rf, rv, out);
}

/* inclusive segmented scan of `in` into out[n] (out may be in.vals). The
 * flags are only read, so a level's flags serve both of its launches. */
static tg_status run_wscan(tg_session* s, PoolScratch& ws, const WscanIn& in, int64_t* out)
{
    if (in.n <= 0) return TG_OK;
    if (in.n <= WSCAN_ONE_WAVE) {
        hipLaunchKernelGGL(k_wscan_one_wave, dim3(1), dim3(64), 0, s->stream, in, out);
        TG_HIP_CHECK(hipGetLastError());
        return TG_OK;
    }
    int64_t nchunks = (in.n + WSCAN_CHUNK - 1) / WSCAN_CHUNK;
    uint8_t* carry_f = nullptr;
    int64_t* carry_v = nullptr;
    TG_TRY(ws.alloc(&carry_f, nchunks));
    TG_TRY(ws.alloc(&carry_v, nchunks * 8));
    int wpb = TG_BLOCK / 64;
    dim3 grid((uint32_t)((nchunks + wpb - 1) / wpb)), block(TG_BLOCK);
    hipLaunchKernelGGL(k_wscan_reduce, grid, block, 0, s->stream, in, nchunks,
                       carry_f, carry_v);
    TG_HIP_CHECK(hipGetLastError());
    WscanIn up{};
    up.vals = carry_v;
    up.flags = carry_f;
    up.n = nchunks;
    up.head_mask = 1;
    up.src = WSRC_ARRAY;
    up.op = in.op;
    TG_TRY(run_wscan(s, ws, up, carry_v));
    hipLaunchKernelGGL(k_wscan_apply, grid, block, 0, s->stream, in, nchunks,
                       (const int64_t*)carry_v, out);
    TG_HIP_CHECK(hipGetLastError());
    return TG_OK;
}

/* the key images of order_pages, as k_win_boundaries reads them */
using WinKey = SortKeyImages;

/* boundary flags of sorted position i against i-1: WFLAG_PARTITION where a
 * partition channel differs, WFLAG_PEER where any channel differs. Equality
 * is equality of image and null bit, i.e. grouping equality. keys[0..n_part)
 * are the partition channels. Position 0 starts both. */
__global__ void k_win_boundaries(const WinKey* __restrict__ keys, int32_t n_keys,
                                 int32_t n_part, const int64_t* __restrict__ perm,
                                 int64_t n, uint8_t* __restrict__ flags)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        int fl = 0;
        if (i == 0) fl = WFLAG_PARTITION | WFLAG_PEER;
        else {
            int64_t a = perm[i - 1], b = perm[i];
            for (int32_t j = 0; j < n_keys; j++) {
                bool differ = keys[j].kf[a] != keys[j].kf[b] ||
                              (keys[j].nf && keys[j].nf[a] != keys[j].nf[b]);
                if (!differ) continue;
                fl = (j < n_part) ? (WFLAG_PARTITION | WFLAG_PEER) : WFLAG_PEER;
                break;   /* partition channels come first */
            }
        }
        flags[i] = (uint8_t)fl;
    }
}

/* aggregate input of one source page in sorted order, widened to i64:
 * vals[o] (0 where NULL) and nonnull[o] (1 / 0) */
template <typename T>
__global__ void k_win_gather_input(const T* __restrict__ src,
                                   const uint64_t* __restrict__ src_valid,
                                   const int64_t* __restrict__ perm, int64_t total,
                                   int64_t base, int64_t n, int64_t* __restrict__ vals,
                                   int64_t* __restrict__ nonnull)
{
    int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; o < total; o += stride) {
        int64_t r = perm[o] - base;
        if (r < 0 || r >= n) continue;
        bool ok = !src_valid || ((src_valid[r >> 6] >> (r & 63)) & 1);
        vals[o] = ok ? (int64_t)src[r] : 0;
        nonnull[o] = ok ? 1 : 0;
    }
}

/* one spec's output column: row i takes the ROWS-frame result at e = end[i]
 * (its own position when end is null); with `count` the cell is NULL unless
 * count[e] > 0. A wave covers 64 aligned rows and writes their validity word
 * with one ballot. */
__global__ void k_win_emit(const int64_t* __restrict__ rows_result,
                           const int64_t* __restrict__ count,
                           const int64_t* __restrict__ end, int64_t n,
                           int64_t* __restrict__ out, uint64_t* __restrict__ out_valid)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t n64 = (n + 63) & ~(int64_t)63;
    for (; i < n64; i += stride) {
        bool ok = false;
        if (i < n) {
            int64_t e = end ? end[i] : i;
            ok = !count || count[e] > 0;
            out[i] = ok ? rows_result[e] : 0;
        }
        if (out_valid) {
            uint64_t w = __ballot(ok);
            if ((threadIdx.x & 63) == 0) out_valid[i >> 6] = w;
        }
    }
}

/* ---- the frame layer: bounded ROWS frames and the value
 * functions. Every frame is an index range [lo, hi] of sorted positions
 * inside the row's partition; an empty frame is stored as (0, -1). ---- */

/* a + b for a >= 0, saturating at INT64_MAX (b < 0 cannot wrap) */
__device__ static inline int64_t win_sat_add(int64_t a, int64_t b)
{
    return b > INT64_MAX - a ? INT64_MAX : a + b;
}

/* frame bounds of every sorted position. ps = i - row_number + 1; `end` is
 * the frame's end index per row for RANGE (last peer) and PARTITION (pe),
 * the partition end for ROWS_BETWEEN, unused for ROWS. */
__global__ void k_win_bounds(int32_t frame, int64_t start, int64_t stop,
                             const int64_t* __restrict__ rownum,
                             const int64_t* __restrict__ end, int64_t n,
                             int64_t* __restrict__ lo, int64_t* __restrict__ hi)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        int64_t l = i - rownum[i] + 1, h = i;
        if (frame == TG_WIN_FRAME_ROWS_BETWEEN) {
            l = max(l, win_sat_add(i, start));
            h = min(end[i], win_sat_add(i, stop));
            if (l > h) {
                l = 0;
                h = -1;
            }
        }
        else if (frame != TG_WIN_FRAME_ROWS) h = end[i];
        lo[i] = l;
        hi[i] = h;
    }
}

/* non-NULL cells of [l, h], a non-empty frame of the partition that starts
 * at ps, from the partition-headed inclusive count */
__device__ static inline int64_t win_frame_count(const int64_t* __restrict__ count,
                                                 int64_t ps, int64_t l, int64_t h)
{
    return count[h] - (l > ps ? count[l - 1] : 0);
}

enum {
    WFE_DIFF = 0,      /* S[hi] - S[lo-1] of a partition-headed scan (wrapping);
                          S null: the frame's row count */
    WFE_AT_HI = 1,     /* S[hi]: a forward min / max scan, frame starts at ps */
    WFE_AT_LO = 2      /* S[lo]: a reverse min / max scan, frame ends at pe */
};

/* one aggregate column over [lo, hi] from scans that exist already. With
 * out_valid the cell is NULL unless the frame holds a non-NULL input. */
__global__ void k_win_frame_emit(int32_t mode, const int64_t* __restrict__ S,
                                 const int64_t* __restrict__ count,
                                 const int64_t* __restrict__ lo,
                                 const int64_t* __restrict__ hi,
                                 const int64_t* __restrict__ rownum, int64_t n,
                                 int64_t* __restrict__ out, uint64_t* __restrict__ out_valid)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t n64 = (n + 63) & ~(int64_t)63;
    for (; i < n64; i += stride) {
        bool ok = false;
        if (i < n) {
            int64_t l = lo[i], h = hi[i], ps = i - rownum[i] + 1, v = 0;
            if (l <= h) {
                ok = !out_valid || win_frame_count(count, ps, l, h) > 0;
                if (mode == WFE_AT_HI) v = S[h];
                else if (mode == WFE_AT_LO) v = S[l];
                else if (!S) v = h - l + 1;
                else v = (int64_t)((uint64_t)S[h] - (uint64_t)(l > ps ? S[l - 1] : 0));
            }
            else ok = !out_valid;      /* an empty frame counts 0 */
            out[i] = ok ? v : 0;
        }
        if (out_valid) {
            uint64_t w = __ballot(ok);
            if ((threadIdx.x & 63) == 0) out_valid[i >> 6] = w;
        }
    }
}

/* sliding min / max over frames bounded at both ends: one level of a sparse
 * table that is never stored. T_0 is the input with NULLs replaced by the
 * identity and T_k[i] = op(T_{k-1}[i], T_{k-1}[i + 2^(k-1)]) covers
 * [i, i + 2^k). Launch k reads T_k (launch 0 reads vals / nonnull), answers
 * every row whose frame length L has floor(log2 L) == k with
 * op(T_k[lo], T_k[hi - 2^k + 1]), and writes T_{k+1} when a later level needs
 * it. The table is not segmented: a frame never leaves its partition, so no
 * query reads a window that does. Launch 0 also writes the whole validity
 * bitmap and the 0 of every NULL cell; later launches read their row's bit.
 * Reads and writes of one launch touch different arrays, and the kernel
 * boundary is the only synchronisation. */
__global__ void k_win_level(int32_t k, int32_t op, const int64_t* __restrict__ T,
                            const int64_t* __restrict__ nonnull, int64_t* __restrict__ Tnext,
                            const int64_t* __restrict__ count,
                            const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                            const int64_t* __restrict__ rownum, int64_t n,
                            int64_t* __restrict__ out, uint64_t* __restrict__ out_valid)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t n64 = (n + 63) & ~(int64_t)63;
    const int64_t ident = wscan_identity(op), w = (int64_t)1 << k;
    /* nonnull is given at level 0 only: T is then the raw input */
    auto cell = [&](int64_t j) { return !nonnull || nonnull[j] ? T[j] : ident; };
    for (; i < n64; i += stride) {
        bool ok = false;
        if (i < n) {
            int64_t l = lo[i], h = hi[i], len = h - l + 1;
            if (k == 0) {
                ok = len > 0 && win_frame_count(count, i - rownum[i] + 1, l, h) > 0;
                if (!ok) out[i] = 0;
            }
            else ok = (out_valid[i >> 6] >> (i & 63)) & 1;
            if (ok && len >= w && (len >> 1) < w)
                out[i] = wscan_op(op, cell(l), cell(h - w + 1));
            if (Tnext) Tnext[i] = wscan_op(op, cell(i), i + w < n ? cell(i + w) : ident);
        }
        if (k == 0) {
            uint64_t b = __ballot(ok);
            if ((threadIdx.x & 63) == 0) out_valid[i >> 6] = b;
        }
    }
}

enum { WVAL_LAG = 0, WVAL_LEAD = 1, WVAL_FIRST = 2, WVAL_LAST = 3, WVAL_NTH = 4 };

/* value functions: row i copies the sorted-order cell at an index computed
 * from its frame (FIRST / LAST / NTH: lo, hi) or its partition (LAG: rownum,
 * LEAD: pend); NULL when the index falls outside or the source cell is NULL.
 * The cells are copied at their own width, bit for bit. */
template <typename T>
__global__ void k_win_value(int32_t mode, int64_t offset, const T* __restrict__ src,
                            const uint64_t* __restrict__ src_valid,
                            const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                            const int64_t* __restrict__ rownum,
                            const int64_t* __restrict__ pend, int64_t n,
                            T* __restrict__ out, uint64_t* __restrict__ out_valid)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t n64 = (n + 63) & ~(int64_t)63;
    for (; i < n64; i += stride) {
        bool ok = false;
        if (i < n) {
            int64_t at = -1;
            if (mode == WVAL_LAG) {
                int64_t j = i - offset;          /* offset >= 0: cannot wrap */
                if (j >= i - rownum[i] + 1) at = j;
            }
            else if (mode == WVAL_LEAD) {
                int64_t j = win_sat_add(i, offset);
                if (j <= pend[i]) at = j;
            }
            else {
                int64_t l = lo[i], h = hi[i];
                if (l <= h) {
                    int64_t j = mode == WVAL_FIRST ? l : mode == WVAL_LAST ? h
                              : win_sat_add(l, offset - 1);
                    if (j <= h) at = j;
                }
            }
            ok = at >= 0 && (!src_valid || ((src_valid[at >> 6] >> (at & 63)) & 1));
            out[i] = ok ? src[at] : (T)0;
        }
        uint64_t w = __ballot(ok);
        if ((threadIdx.x & 63) == 0) out_valid[i >> 6] = w;
    }
}

struct WindowOp : tg_operator {
    std::vector<tg_type> types;
    std::vector<int32_t> partition_channels;
    std::vector<int32_t> sort_channels;
    std::vector<int32_t> sort_desc;     /* 0 asc, 1 desc */
    std::vector<tg_window_spec_ex> specs;
    std::vector<DevPage> pages;
    int64_t total_rows = 0;
    bool emitted = false;

    tg_status add_input(const tg_page* page) override
    {
        TG_TRY(check_fixed_width_page("window", page, types));
        DevPage in;
        TG_TRY(tg_upload_page(s, page, &in));
        total_rows += in.n;
        pages.emplace_back(std::move(in));
        return TG_OK;
    }

    static bool is_ranking(int32_t fn) { return fn <= TG_WIN_DENSE_RANK; }
    static bool has_validity(int32_t fn) { return fn >= TG_WIN_SUM_I64; }
    static bool is_value_fn(int32_t fn) { return fn >= TG_WIN_LAG; }
    static bool is_aggregate(int32_t fn) { return fn >= TG_WIN_COUNT_COL && fn <= TG_WIN_MAX_I64; }

    /* launches of k_win_level for ROWS BETWEEN start AND stop over n rows: a
     * frame holds at most min(stop - start + 1, n) rows, and a frame of L
     * rows is answered at level floor(log2 L). One launch always runs: it
     * writes the bitmap. */
    static int32_t window_levels(int64_t start, int64_t stop, int64_t n)
    {
        if (stop < start) return 1;
        uint64_t width = (uint64_t)stop - (uint64_t)start + 1;     /* no wrap: both bounded */
        uint64_t longest = width < (uint64_t)n ? width : (uint64_t)n;
        int32_t levels = 1;
        while (longest >>= 1) levels++;
        return levels;
    }

    tg_status launch_value(int32_t mode, int64_t offset, const DevBlock& src,
                           const int64_t* lo, const int64_t* hi, const int64_t* rn,
                           const int64_t* pend, DevBlock& b)
    {
        dim3 grid(tg_grid_for(total_rows)), block(TG_BLOCK);
        tg_dispatch_width(b.elem_size(), [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_win_value<T>, grid, block, 0, s->stream, mode, offset,
                               (const T*)src.data, (const uint64_t*)src.valid, lo, hi, rn, pend,
                               total_rows, (T*)b.data, b.valid);
        });
        TG_HIP_CHECK(hipGetLastError());
        return TG_OK;
    }

    /* aggregate input of channel ch in sorted order */
    tg_status gather_input(PoolScratch& ws, const std::vector<int64_t>& page_base,
                           const int64_t* d_perm, int32_t ch, int64_t** vals_out,
                           int64_t** nonnull_out)
    {
        int64_t *vals = nullptr, *nonnull = nullptr;
        TG_TRY(ws.alloc(&vals, total_rows * 8));
        TG_TRY(ws.alloc(&nonnull, total_rows * 8));
        dim3 grid(tg_grid_for(total_rows)), block(TG_BLOCK);
        for (size_t p = 0; p < pages.size(); p++) {
            const DevBlock& sb = pages[p].blocks[ch];
            int64_t pn = pages[p].n;
            if (!pn) continue;
            tg_dispatch_width(sb.elem_size(), [&](auto t) {
                using T = decltype(t);
                hipLaunchKernelGGL(k_win_gather_input<T>, grid, block, 0, s->stream,
                                   (const T*)sb.data, sb.valid, d_perm, total_rows,
                                   page_base[p], pn, vals, nonnull);
            });
            TG_HIP_CHECK(hipGetLastError());
        }
        *vals_out = vals;
        *nonnull_out = nonnull;
        return TG_OK;
    }

    tg_status emit_into(PoolScratch& ws, DevPage* outp)
    {
        const int64_t n = total_rows;
        std::vector<int64_t> page_base(pages.size() + 1, 0);
        for (size_t p = 0; p < pages.size(); p++)
            page_base[p + 1] = page_base[p] + pages[p].n;

        int64_t* d_perm = nullptr;
        TG_TRY(ws.alloc(&d_perm, n * 8));
        /* partition channels first (ASC NULLS LAST), then the sort channels;
         * the key images stay alive in the scratch for the boundary kernel */
        std::vector<std::pair<int32_t, int32_t>> keys;
        for (int32_t ch : partition_channels) keys.emplace_back(ch, 0);
        for (size_t j = 0; j < sort_channels.size(); j++)
            keys.emplace_back(sort_channels[j], sort_desc[j] != 0);
        std::vector<WinKey> host_keys;
        TG_TRY(order_pages(s, ws, pages, n, keys, d_perm, &host_keys));

        /* partition-start and peer-start bits of every sorted position */
        uint8_t* d_flags = nullptr;
        WinKey* d_keytab = nullptr;
        TG_TRY(ws.alloc(&d_flags, n));
        TG_TRY(ws.alloc(&d_keytab, (int64_t)(host_keys.size() * sizeof(WinKey))));
        if (!host_keys.empty()) {
            TG_HIP_CHECK(hipMemcpyAsync(d_keytab, host_keys.data(),
                                        host_keys.size() * sizeof(WinKey),
                                        hipMemcpyHostToDevice, s->stream));
            TG_HIP_CHECK(hipStreamSynchronize(s->stream));   /* host_keys is a local */
        }
        hipLaunchKernelGGL(k_win_boundaries, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0,
                           s->stream, (const WinKey*)d_keytab, (int32_t)host_keys.size(),
                           (int32_t)partition_channels.size(), (const int64_t*)d_perm, n,
                           d_flags);
        TG_HIP_CHECK(hipGetLastError());

        /* every input channel through the final permutation */
        TG_TRY(gather_pages(s, pages, types, d_perm, n, outp));

        /* intermediates shared by the specs, each computed at most once */
        int64_t* d_rownum = nullptr;
        int64_t* d_end[3] = {nullptr, nullptr, nullptr};       /* by frame */
        struct Input { int64_t *vals, *nonnull, *count; };
        std::map<int32_t, Input> inputs;                        /* by channel */

        auto scan = [&](int32_t src, int32_t op, int32_t head_mask, int32_t val_mask,
                        const int64_t* vals, const int64_t* aux, int32_t reverse,
                        int64_t* out) {
            WscanIn in{};
            in.vals = vals;
            in.aux = aux;
            in.flags = d_flags;
            in.n = n;
            in.head_mask = head_mask;
            in.val_mask = val_mask;
            in.src = src;
            in.op = op;
            in.reverse = reverse;
            return run_wscan(s, ws, in, out);
        };
        auto rownum = [&]() -> tg_status {
            if (d_rownum) return TG_OK;
            TG_TRY(ws.alloc(&d_rownum, n * 8));
            return scan(WSRC_ONE, WOP_ADD, WFLAG_PARTITION, 0, nullptr, nullptr, 0, d_rownum);
        };
        /* index of the last row of the peer group (RANGE) or partition */
        auto frame_end = [&](int32_t frame) -> tg_status {
            if (frame == TG_WIN_FRAME_ROWS || d_end[frame]) return TG_OK;
            TG_TRY(ws.alloc(&d_end[frame], n * 8));
            int32_t mask = frame == TG_WIN_FRAME_RANGE ? WFLAG_PEER : WFLAG_PARTITION;
            return scan(WSRC_INDEX, WOP_MAX, mask, 0, nullptr, nullptr, 1, d_end[frame]);
        };
        auto input = [&](int32_t ch) -> tg_status {
            if (inputs.count(ch)) return TG_OK;
            Input in{nullptr, nullptr, nullptr};
            TG_TRY(gather_input(ws, page_base, d_perm, ch, &in.vals, &in.nonnull));
            TG_TRY(ws.alloc(&in.count, n * 8));
            TG_TRY(scan(WSRC_ARRAY, WOP_ADD, WFLAG_PARTITION, 0, in.nonnull, nullptr, 0,
                        in.count));
            inputs[ch] = in;
            return TG_OK;
        };

        /* the frame layer's intermediates, each at most once per operator:
         * [lo, hi] per distinct frame, and the NULL-neutralised partition-
         * headed scans of an input by (channel, op, direction) */
        struct Bounds { int64_t *lo, *hi; };
        std::map<std::tuple<int32_t, int64_t, int64_t>, Bounds> bounds;
        std::map<std::tuple<int32_t, int32_t, int32_t>, int64_t*> runnings;
        auto frame_bounds = [&](const tg_window_spec_ex& sp, Bounds* got) -> tg_status {
            auto key = std::make_tuple(sp.frame, sp.frame_start, sp.frame_end);
            auto it = bounds.find(key);
            if (it != bounds.end()) {
                *got = it->second;
                return TG_OK;
            }
            /* ROWS_BETWEEN clamps at the partition end */
            int32_t endf = sp.frame == TG_WIN_FRAME_ROWS_BETWEEN ? (int32_t)TG_WIN_FRAME_PARTITION
                                                                 : sp.frame;
            TG_TRY(rownum());
            TG_TRY(frame_end(endf));
            Bounds b{nullptr, nullptr};
            TG_TRY(ws.alloc(&b.lo, n * 8));
            TG_TRY(ws.alloc(&b.hi, n * 8));
            hipLaunchKernelGGL(k_win_bounds, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0, s->stream,
                               sp.frame, sp.frame_start, sp.frame_end,
                               (const int64_t*)d_rownum, (const int64_t*)d_end[endf], n,
                               b.lo, b.hi);
            TG_HIP_CHECK(hipGetLastError());
            bounds[key] = b;
            *got = b;
            return TG_OK;
        };
        auto running = [&](int32_t ch, int32_t op, int32_t reverse, int64_t** got) -> tg_status {
            auto key = std::make_tuple(ch, op, reverse);
            auto it = runnings.find(key);
            if (it != runnings.end()) {
                *got = it->second;
                return TG_OK;
            }
            const Input& in = inputs[ch];
            int64_t* r = nullptr;
            TG_TRY(ws.alloc(&r, n * 8));
            TG_TRY(scan(WSRC_NEUTRAL, op, WFLAG_PARTITION, 0, in.vals, in.nonnull, reverse, r));
            runnings[key] = r;
            *got = r;
            return TG_OK;
        };

        for (const tg_window_spec_ex& sp : specs) {
            outp->blocks.emplace_back();
            DevBlock& b = outp->blocks.back();
            b.type = is_value_fn(sp.fn) ? types[sp.input_channel] : TG_BIGINT;
            b.n = n;
            TG_POOL_ALLOC(s, &b.data, n * b.elem_size());
            if (has_validity(sp.fn)) TG_POOL_ALLOC(s, &b.valid, ((n + 63) / 64) * 8);
            int64_t* out = (int64_t*)b.data;
            if (is_value_fn(sp.fn)) {
                /* the cells in sorted order are the payload channel itself */
                const DevBlock& src = outp->blocks[sp.input_channel];
                Bounds fb{nullptr, nullptr};
                if (sp.fn == TG_WIN_LAG) TG_TRY(rownum());
                else if (sp.fn == TG_WIN_LEAD) TG_TRY(frame_end(TG_WIN_FRAME_PARTITION));
                else TG_TRY(frame_bounds(sp, &fb));
                TG_TRY(launch_value(sp.fn - TG_WIN_LAG, sp.offset, src, fb.lo, fb.hi, d_rownum,
                                    d_end[TG_WIN_FRAME_PARTITION], b));
                continue;
            }
            if (sp.frame == TG_WIN_FRAME_ROWS_BETWEEN) {
                Bounds fb{nullptr, nullptr};
                TG_TRY(frame_bounds(sp, &fb));
                dim3 grid(tg_grid_for(n)), block(TG_BLOCK);
                if (sp.fn == TG_WIN_COUNT_STAR) {
                    hipLaunchKernelGGL(k_win_frame_emit, grid, block, 0, s->stream,
                                       (int32_t)WFE_DIFF, (const int64_t*)nullptr,
                                       (const int64_t*)nullptr, (const int64_t*)fb.lo,
                                       (const int64_t*)fb.hi, (const int64_t*)d_rownum, n, out,
                                       (uint64_t*)nullptr);
                    TG_HIP_CHECK(hipGetLastError());
                    continue;
                }
                TG_TRY(input(sp.input_channel));
                const Input in = inputs[sp.input_channel];
                int32_t op = sp.fn == TG_WIN_MIN_I64 ? WOP_MIN
                           : sp.fn == TG_WIN_MAX_I64 ? WOP_MAX : WOP_ADD;
                /* an offset that reaches past every partition is unbounded */
                bool open_start = sp.frame_start <= -(n - 1);
                bool open_end = sp.frame_end >= n - 1;
                if (op == WOP_ADD || open_start || open_end) {
                    /* prefix difference, or a min / max scan read at one end */
                    int32_t mode = op == WOP_ADD ? WFE_DIFF : open_start ? WFE_AT_HI : WFE_AT_LO;
                    const int64_t* S = in.count;
                    if (sp.fn != TG_WIN_COUNT_COL) {
                        int64_t* r = nullptr;
                        TG_TRY(running(sp.input_channel, op, mode == WFE_AT_LO, &r));
                        S = r;
                    }
                    hipLaunchKernelGGL(k_win_frame_emit, grid, block, 0, s->stream, mode, S,
                                       (const int64_t*)in.count, (const int64_t*)fb.lo,
                                       (const int64_t*)fb.hi, (const int64_t*)d_rownum, n, out,
                                       b.valid);
                    TG_HIP_CHECK(hipGetLastError());
                    continue;
                }
                /* sliding min / max: one launch per level of the widest frame */
                int32_t levels = window_levels(sp.frame_start, sp.frame_end, n);
                int64_t* T[2] = {nullptr, nullptr};
                for (int t = 0; t < 2 && t < levels - 1; t++) TG_TRY(ws.alloc(&T[t], n * 8));
                for (int32_t k = 0; k < levels; k++) {
                    const int64_t* src = k ? T[(k - 1) & 1] : in.vals;
                    hipLaunchKernelGGL(k_win_level, grid, block, 0, s->stream, k, op, src,
                                       (const int64_t*)(k ? nullptr : in.nonnull),
                                       k + 1 < levels ? T[k & 1] : (int64_t*)nullptr,
                                       (const int64_t*)in.count, (const int64_t*)fb.lo,
                                       (const int64_t*)fb.hi, (const int64_t*)d_rownum, n, out,
                                       b.valid);
                    TG_HIP_CHECK(hipGetLastError());
                }
                continue;
            }
            if (sp.fn == TG_WIN_RANK) {
                TG_TRY(rownum());
                TG_TRY(scan(WSRC_MASKED, WOP_MAX, WFLAG_PARTITION, WFLAG_PEER, d_rownum,
                            nullptr, 0, out));
                continue;
            }
            if (sp.fn == TG_WIN_DENSE_RANK) {
                TG_TRY(scan(WSRC_FLAG, WOP_ADD, WFLAG_PARTITION, WFLAG_PEER, nullptr,
                            nullptr, 0, out));
                continue;
            }
            /* the ROWS-frame result, then the frame's gather */
            const int64_t* rows_result = nullptr;
            const int64_t* count = nullptr;
            if (sp.fn == TG_WIN_ROW_NUMBER || sp.fn == TG_WIN_COUNT_STAR) {
                TG_TRY(rownum());
                rows_result = d_rownum;
            }
            else {
                TG_TRY(input(sp.input_channel));
                const Input& in = inputs[sp.input_channel];
                if (sp.fn == TG_WIN_COUNT_COL) rows_result = in.count;
                else {
                    int32_t op = sp.fn == TG_WIN_SUM_I64 ? WOP_ADD
                               : sp.fn == TG_WIN_MIN_I64 ? WOP_MIN : WOP_MAX;
                    int64_t* r = nullptr;
                    TG_TRY(ws.alloc(&r, n * 8));
                    TG_TRY(scan(WSRC_NEUTRAL, op, WFLAG_PARTITION, 0, in.vals, in.nonnull,
                                0, r));
                    rows_result = r;
                    count = in.count;
                }
            }
            /* row_number has no frame: its frame field is 0 by contract */
            int32_t frame = sp.fn == TG_WIN_ROW_NUMBER ? TG_WIN_FRAME_ROWS : sp.frame;
            TG_TRY(frame_end(frame));
            hipLaunchKernelGGL(k_win_emit, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0, s->stream,
                               rows_result, count, (const int64_t*)d_end[frame], n, out,
                               b.valid);
            TG_HIP_CHECK(hipGetLastError());
        }
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        return TG_OK;
    }

    tg_status emit()
    {
        if (total_rows) {
            DevPage outp;
            tg_status st;
            {
                PoolScratch ws(s);
                st = emit_into(ws, &outp);
            }   /* the scratch is back in the pool, the stream drained */
            if (st != TG_OK) {
                tg_free_page(s, &outp);
                return st;
            }
            stage_output(std::move(outp));
        }
        for (auto& p : pages) tg_free_page(s, &p);
        pages.clear();
        return TG_OK;
    }

    tg_status get_output(tg_page* out, int* finished) override
    {
        if (input_finished && !emitted) {
            emitted = true;
            tg_status st = emit();
            if (st != TG_OK) return st;
        }
        emit_staged(out, finished);
        return TG_OK;
    }

    ~WindowOp() override
    {
        for (auto& p : pages) tg_free_page(s, &p);
        for (auto& p : out_pages_) tg_free_page(s, &p);
    }
};

static tg_window_spec_ex window_widen(const tg_window_spec& sp)
{
    return tg_window_spec_ex{sp.fn, sp.input_channel, sp.frame, 0, 0, 0, 0};
}
static tg_window_spec_ex window_widen(const tg_window_spec_ex& sp) { return sp; }

/* both entry points: the same checks in the same order, with the functions
 * and frames up to max_fn / max_frame */
template <typename Spec>
static tg_status window_create(tg_session* s,
    const int32_t* types, int32_t n_channels,
    const int32_t* partition_channels, int32_t n_partition,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    const Spec* specs, int32_t n_specs, int32_t max_fn, int32_t max_frame, tg_operator** out)
{
    if (!s || !types || !out || n_channels < 1 || n_partition < 0 || n_sort < 0 ||
        (n_partition && !partition_channels) || (n_sort && (!sort_channels || !sort_desc)) ||
        !specs) {
        TG_SET_ERR("invalid window spec: null argument or negative count");
        return TG_ERR_INVALID_ARG;
    }
    if (n_specs < 1 || n_specs > 8) {
        TG_SET_ERR("window: %d specs, 1..8 supported", n_specs);
        return TG_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n_partition; i++)
        if (partition_channels[i] < 0 || partition_channels[i] >= n_channels) {
            TG_SET_ERR("window partition channel %d outside %d channels",
                       partition_channels[i], n_channels);
            return TG_ERR_INVALID_ARG;
        }
    for (int i = 0; i < n_sort; i++)
        if (sort_channels[i] < 0 || sort_channels[i] >= n_channels) {
            TG_SET_ERR("window sort channel %d outside %d channels", sort_channels[i], n_channels);
            return TG_ERR_INVALID_ARG;
        }
    std::vector<tg_window_spec_ex> wide;
    for (int i = 0; i < n_specs; i++) wide.push_back(window_widen(specs[i]));
    for (int i = 0; i < n_specs; i++) {
        const tg_window_spec_ex& sp = wide[i];
        if (sp.fn < TG_WIN_ROW_NUMBER || sp.fn > max_fn) {
            TG_SET_ERR("window spec %d: unknown function %d", i, sp.fn);
            return TG_ERR_INVALID_ARG;
        }
        if (sp.frame < TG_WIN_FRAME_RANGE || sp.frame > max_frame) {
            TG_SET_ERR("window spec %d: unknown frame %d", i, sp.frame);
            return TG_ERR_INVALID_ARG;
        }
        bool positional = sp.fn == TG_WIN_LAG || sp.fn == TG_WIN_LEAD;
        if ((WindowOp::is_ranking(sp.fn) || positional) && sp.frame != TG_WIN_FRAME_RANGE) {
            TG_SET_ERR("window spec %d: %s function %d takes frame 0, not %d", i,
                       positional ? "lag / lead" : "ranking", sp.fn, sp.frame);
            return TG_ERR_INVALID_ARG;
        }
        if (sp.fn >= TG_WIN_COUNT_COL &&
            (sp.input_channel < 0 || sp.input_channel >= n_channels)) {
            TG_SET_ERR("window spec %d: input channel %d outside %d channels", i,
                       sp.input_channel, n_channels);
            return TG_ERR_INVALID_ARG;
        }
        if (sp.frame != TG_WIN_FRAME_ROWS_BETWEEN && (sp.frame_start || sp.frame_end)) {
            TG_SET_ERR("window spec %d: frame offsets with frame %d; only ROWS_BETWEEN takes them",
                       i, sp.frame);
            return TG_ERR_INVALID_ARG;
        }
        if (sp.frame_start == TG_WIN_UNBOUNDED_FOLLOWING ||
            sp.frame_end == TG_WIN_UNBOUNDED_PRECEDING) {
            TG_SET_ERR("window spec %d: a frame starts at UNBOUNDED FOLLOWING or ends at "
                       "UNBOUNDED PRECEDING", i);
            return TG_ERR_INVALID_ARG;
        }
        if (sp.offset && !positional && sp.fn != TG_WIN_NTH_VALUE) {
            TG_SET_ERR("window spec %d: function %d takes no offset", i, sp.fn);
            return TG_ERR_INVALID_ARG;
        }
        if ((positional && sp.offset < 0) || (sp.fn == TG_WIN_NTH_VALUE && sp.offset < 1)) {
            TG_SET_ERR("window spec %d: offset %lld of function %d", i, (long long)sp.offset,
                       sp.fn);
            return TG_ERR_INVALID_ARG;
        }
    }
    /* the payload gather moves fixed-width cells only (as TopN) */
    for (int i = 0; i < n_channels; i++)
        if (types[i] == TG_VARCHAR) {
            TG_SET_ERR("window: VARCHAR channel %d is not supported", i);
            return TG_ERR_UNSUPPORTED;
        }
    /* a parallel scan reassociates the additions: exact for integers only.
     * The value functions copy cells and take a DOUBLE channel. */
    for (int i = 0; i < n_specs; i++)
        if (WindowOp::is_aggregate(wide[i].fn) && types[wide[i].input_channel] == TG_DOUBLE) {
            TG_SET_ERR("window spec %d: DOUBLE input channel %d is not supported", i,
                       wide[i].input_channel);
            return TG_ERR_UNSUPPORTED;
        }
    auto* op = new WindowOp();
    op->s = s;
    for (int i = 0; i < n_channels; i++) op->types.push_back((tg_type)types[i]);
    op->partition_channels.assign(partition_channels, partition_channels + n_partition);
    op->sort_channels.assign(sort_channels, sort_channels + n_sort);
    op->sort_desc.assign(sort_desc, sort_desc + n_sort);
    op->specs = std::move(wide);
    *out = op;
    return TG_OK;
}

extern "C" tg_status tg_window_create(tg_session* s,
    const int32_t* types, int32_t n_channels,
    const int32_t* partition_channels, int32_t n_partition,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    const tg_window_spec* specs, int32_t n_specs, tg_operator** out)
{
    return window_create(s, types, n_channels, partition_channels, n_partition, sort_channels,
                         sort_desc, n_sort, specs, n_specs, TG_WIN_MAX_I64,
                         TG_WIN_FRAME_PARTITION, out);
}

extern "C" tg_status tg_window_create_ex(tg_session* s,
    const int32_t* types, int32_t n_channels,
    const int32_t* partition_channels, int32_t n_partition,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    const tg_window_spec_ex* specs, int32_t n_specs, tg_operator** out)
{
    return window_create(s, types, n_channels, partition_channels, n_partition, sort_channels,
                         sort_desc, n_sort, specs, n_specs, TG_WIN_NTH_VALUE,
                         TG_WIN_FRAME_ROWS_BETWEEN, out);
}

/* ---- TopNRanking (operator/TopNRankingOperator.java analog):
 * the rows of `row_number() / rank() / dense_rank() OVER (PARTITION BY ...
 * ORDER BY ...) <= N`, without the Window's n-row payload gather and n-row
 * ranking column. Input pages are staged; a COMPACTION orders the retained
 * page and the staged pages together (order_pages, the retained page first,
 * so stability keeps earlier input ahead of later input among ties), marks
 * the boundaries (k_win_boundaries), computes the ranking with the scan the
 * Window uses for that function (run_wscan), cuts at N (the rank cut below)
 * and gathers ONLY the kept rows into the new retained page. add_input
 * compacts whenever the buffered rows reach max(threshold, 2 x the rows the
 * last compaction retained), which bounds memory by the threshold plus the
 * kept rows and keeps the total work linear when nothing can be cut; finish
 * compacts once more if rows were staged since, and emits the retained page
 * with the rankings that compaction placed. Pruning is exact: a row
 * cut over a subset of the input is cut over the whole input, and no kept
 * row loses a row that counts towards its ranking (§6i).
 *
 * The rank cut is an ordered compaction in the no-waiting shape of the scan:
 * a wave per WSCAN_CHUNK rows counts its keeps (one ballot and popcount per
 * 64-row group), the per-chunk counts are scanned by run_wscan, and the same
 * chunk pass runs again placing each kept row at base[chunk] + the keeps in
 * the lanes below it. No atomics, no look-back, no flag polling; no block
 * waits on another, so placement is deterministic and order-preserving. ---- */

/* keeps of 64-row group k of a batch: rows [g + 64k, ...) below hi whose
 * ranking is <= limit. WSCAN_BATCH groups are loaded before the first ballot,
 * as in wscan_chunk. */
__device__ static inline void rcut_load(const int64_t* __restrict__ ranking, int64_t g,
                                        int64_t hi, int lane, int64_t limit,
                                        int64_t (&rk)[WSCAN_BATCH], bool (&keep)[WSCAN_BATCH])
{
    #pragma unroll
    for (int k = 0; k < WSCAN_BATCH; k++) {
        int64_t p = g + 64 * k + lane;
        rk[k] = p < hi ? ranking[p] : INT64_MAX;
        keep[k] = p < hi && rk[k] <= limit;
    }
}

/* launch 1: chunk c -> the number of its kept rows */
__global__ void k_rcut_count(const int64_t* __restrict__ ranking, int64_t n, int64_t limit,
                             int64_t nchunks, int64_t* __restrict__ counts)
{
    int64_t c = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (c >= nchunks) return;
    int lane = threadIdx.x % 64;
    int64_t lo = c * WSCAN_CHUNK, hi = min(lo + (int64_t)WSCAN_CHUNK, n);
    int64_t kept = 0;
    for (int64_t g = lo; g < hi; g += 64 * WSCAN_BATCH) {
        int64_t rk[WSCAN_BATCH];
        bool keep[WSCAN_BATCH];
        rcut_load(ranking, g, hi, lane, limit, rk, keep);
        #pragma unroll
        for (int k = 0; k < WSCAN_BATCH; k++) kept += __popcll(__ballot(keep[k]));
    }
    if (lane == 0) counts[c] = kept;
}

/* launch 3: the chunk pass again. counts_scanned is the INCLUSIVE scan of the
 * counts, so chunk c starts at counts_scanned[c - 1]; a kept row lands at that
 * base + the keeps before it in its chunk. kept_rank may be null. Every write
 * lies below counts_scanned[nchunks - 1], the size of both outputs: the keep
 * test is the one launch 1 counted. */
__global__ void k_rcut_place(const int64_t* __restrict__ ranking,
                             const int64_t* __restrict__ perm, int64_t n, int64_t limit,
                             int64_t nchunks, const int64_t* __restrict__ counts_scanned,
                             int64_t* __restrict__ kept_idx, int64_t* __restrict__ kept_rank)
{
    int64_t c = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (c >= nchunks) return;
    int lane = threadIdx.x % 64;
    int64_t lo = c * WSCAN_CHUNK, hi = min(lo + (int64_t)WSCAN_CHUNK, n);
    int64_t base = c ? counts_scanned[c - 1] : 0;
    const uint64_t below = (1ull << lane) - 1ull;
    for (int64_t g = lo; g < hi; g += 64 * WSCAN_BATCH) {
        int64_t rk[WSCAN_BATCH];
        bool keep[WSCAN_BATCH];
        rcut_load(ranking, g, hi, lane, limit, rk, keep);
        #pragma unroll
        for (int k = 0; k < WSCAN_BATCH; k++) {
            uint64_t b = __ballot(keep[k]);
            if (keep[k]) {
                int64_t at = base + __popcll(b & below);
                kept_idx[at] = perm[g + 64 * k + lane];
                if (kept_rank) kept_rank[at] = rk[k];
            }
            base += __popcll(b);
        }
    }
}

struct TopNRankingOp : tg_operator {
    std::vector<tg_type> types;
    std::vector<int32_t> partition_channels;
    std::vector<int32_t> sort_channels;
    std::vector<int32_t> sort_desc;     /* 0 asc, 1 desc */
    int32_t fn = TG_RANKING_ROW_NUMBER;
    int64_t limit = 1;
    bool emit_ranking = true;
    int64_t threshold = 0;
    /* after a compaction pages[0] is the retained page; the rest is staged */
    std::vector<DevPage> pages;
    /* with emit_ranking: the rankings of the retained page's rows, true for
     * the input so far; finish emits them as they are when nothing was
     * staged after the last compaction */
    DevBlock retained_rank;
    int64_t buffered_rows = 0;
    int64_t staged_rows = 0;
    int64_t last_retained = 0;
    bool emitted = false;

    tg_status add_input(const tg_page* page) override
    {
        TG_TRY(check_fixed_width_page("topn_ranking", page, types));
        DevPage in;
        TG_TRY(tg_upload_page(s, page, &in));
        buffered_rows += in.n;
        staged_rows += in.n;
        pages.emplace_back(std::move(in));
        if (buffered_rows >= std::max(threshold, 2 * last_retained)) return compact();
        return TG_OK;
    }

    void free_rank()
    {
        if (retained_rank.data) tg_pool_free(s, retained_rank.data);
        retained_rank.data = nullptr;
    }

    /* the ranking of every sorted position into d_rank, by the Window's scans */
    tg_status ranking(PoolScratch& ws, const uint8_t* d_flags, int64_t n, int64_t* d_rank)
    {
        auto scan = [&](int32_t src, int32_t op, int32_t val_mask, const int64_t* vals,
                        int64_t* out) {
            WscanIn in{};
            in.vals = vals;
            in.flags = d_flags;
            in.n = n;
            in.head_mask = WFLAG_PARTITION;
            in.val_mask = val_mask;
            in.src = src;
            in.op = op;
            return run_wscan(s, ws, in, out);
        };
        if (fn == TG_RANKING_DENSE_RANK) return scan(WSRC_FLAG, WOP_ADD, WFLAG_PEER, nullptr, d_rank);
        if (fn == TG_RANKING_ROW_NUMBER) return scan(WSRC_ONE, WOP_ADD, 0, nullptr, d_rank);
        /* RANK: the row number of the row's first peer */
        int64_t* d_rownum = nullptr;
        TG_TRY(ws.alloc(&d_rownum, n * 8));
        TG_TRY(scan(WSRC_ONE, WOP_ADD, 0, nullptr, d_rownum));
        return scan(WSRC_MASKED, WOP_MAX, WFLAG_PEER, d_rownum, d_rank);
    }

    /* (pages) -> the page of their rows with ranking <= limit in sorted
     * order; with rank_out also the BIGINT ranking block of those rows */
    tg_status compact_into(PoolScratch& ws, DevPage* outp, DevBlock* rank_out)
    {
        const int64_t n = buffered_rows;
        int64_t* d_perm = nullptr;
        TG_TRY(ws.alloc(&d_perm, n * 8));
        std::vector<std::pair<int32_t, int32_t>> keys;
        for (int32_t ch : partition_channels) keys.emplace_back(ch, 0);
        for (size_t j = 0; j < sort_channels.size(); j++)
            keys.emplace_back(sort_channels[j], sort_desc[j] != 0);
        std::vector<WinKey> host_keys;
        TG_TRY(order_pages(s, ws, pages, n, keys, d_perm, &host_keys));

        uint8_t* d_flags = nullptr;
        WinKey* d_keytab = nullptr;
        TG_TRY(ws.alloc(&d_flags, n));
        TG_TRY(ws.alloc(&d_keytab, (int64_t)(host_keys.size() * sizeof(WinKey))));
        if (!host_keys.empty()) {
            TG_HIP_CHECK(hipMemcpyAsync(d_keytab, host_keys.data(),
                                        host_keys.size() * sizeof(WinKey),
                                        hipMemcpyHostToDevice, s->stream));
            TG_HIP_CHECK(hipStreamSynchronize(s->stream));   /* host_keys is a local */
        }
        hipLaunchKernelGGL(k_win_boundaries, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0,
                           s->stream, (const WinKey*)d_keytab, (int32_t)host_keys.size(),
                           (int32_t)partition_channels.size(), (const int64_t*)d_perm, n,
                           d_flags);
        TG_HIP_CHECK(hipGetLastError());

        int64_t* d_rank = nullptr;
        TG_TRY(ws.alloc(&d_rank, n * 8));
        TG_TRY(ranking(ws, d_flags, n, d_rank));

        /* the rank cut: count, scan the counts, place */
        int64_t nchunks = (n + WSCAN_CHUNK - 1) / WSCAN_CHUNK;
        int64_t* d_counts = nullptr;
        uint8_t* d_noheads = nullptr;
        TG_TRY(ws.alloc(&d_counts, nchunks * 8));
        TG_TRY(ws.alloc(&d_noheads, nchunks));
        int wpb = TG_BLOCK / 64;
        dim3 grid((uint32_t)((nchunks + wpb - 1) / wpb)), block(TG_BLOCK);
        hipLaunchKernelGGL(k_rcut_count, grid, block, 0, s->stream, (const int64_t*)d_rank, n,
                           limit, nchunks, d_counts);
        TG_HIP_CHECK(hipGetLastError());
        WscanIn sum{};
        sum.vals = d_counts;
        sum.flags = d_noheads;      /* read, never used: head_mask is 0 */
        sum.n = nchunks;
        sum.src = WSRC_ARRAY;
        sum.op = WOP_ADD;
        TG_HIP_CHECK(hipMemsetAsync(d_noheads, 0, nchunks, s->stream));
        TG_TRY(run_wscan(s, ws, sum, d_counts));
        int64_t m = 0;
        TG_HIP_CHECK(hipMemcpyAsync(&m, d_counts + (nchunks - 1), 8, hipMemcpyDeviceToHost,
                                    s->stream));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        if (m < 1 || m > n) {     /* every partition keeps its first row */
            TG_SET_ERR("topn_ranking: the rank cut kept %lld of %lld rows", (long long)m,
                       (long long)n);
            return TG_ERR_HIP;
        }
        int64_t* d_kept = nullptr;
        TG_TRY(ws.alloc(&d_kept, m * 8));
        if (rank_out) {
            rank_out->type = TG_BIGINT;
            rank_out->n = m;
            TG_POOL_ALLOC(s, &rank_out->data, m * 8);
        }
        hipLaunchKernelGGL(k_rcut_place, grid, block, 0, s->stream, (const int64_t*)d_rank,
                           (const int64_t*)d_perm, n, limit, nchunks,
                           (const int64_t*)d_counts, d_kept,
                           rank_out ? (int64_t*)rank_out->data : (int64_t*)nullptr);
        TG_HIP_CHECK(hipGetLastError());

        /* only kept rows have their payload moved */
        TG_TRY(gather_pages(s, pages, types, d_kept, m, outp));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        return TG_OK;
    }

    /* reduce (retained page, staged pages) to one retained page */
    tg_status compact()
    {
        DevPage outp;
        DevBlock rank;
        tg_status st;
        {
            PoolScratch ws(s);
            st = compact_into(ws, &outp, emit_ranking ? &rank : nullptr);
        }   /* the scratch is back in the pool, the stream drained */
        if (st != TG_OK) {
            tg_free_page(s, &outp);
            if (rank.data) tg_pool_free(s, rank.data);
            return st;
        }
        for (auto& p : pages) tg_free_page(s, &p);
        pages.clear();
        free_rank();
        retained_rank = rank;
        buffered_rows = last_retained = outp.n;
        staged_rows = 0;
        pages.emplace_back(std::move(outp));
        return TG_OK;
    }

    tg_status emit()
    {
        /* rows staged after the last compaction: one more; otherwise the
         * retained page and its rankings are the result already */
        if (staged_rows) TG_TRY(compact());
        if (buffered_rows) {
            DevPage outp = std::move(pages[0]);
            if (emit_ranking) {
                outp.blocks.emplace_back(retained_rank);
                retained_rank.data = nullptr;       /* the page owns it now */
            }
            stage_output(std::move(outp));
            buffered_rows = 0;
        }
        for (auto& p : pages) tg_free_page(s, &p);         /* zero-row pages */
        pages.clear();
        return TG_OK;
    }

    tg_status get_output(tg_page* out, int* finished) override
    {
        if (input_finished && !emitted) {
            emitted = true;
            tg_status st = emit();
            if (st != TG_OK) return st;
        }
        emit_staged(out, finished);
        return TG_OK;
    }

    ~TopNRankingOp() override
    {
        free_rank();
        for (auto& p : pages) tg_free_page(s, &p);
        for (auto& p : out_pages_) tg_free_page(s, &p);
    }
};

extern "C" tg_status tg_topn_ranking_create(tg_session* s,
    const int32_t* types, int32_t n_channels,
    const int32_t* partition_channels, int32_t n_partition,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    int32_t ranking_fn, int32_t max_ranking_per_partition, int32_t emit_ranking,
    tg_operator** out)
{
    if (!s || !types || !out || n_channels < 1 || n_partition < 0 || n_sort < 0 ||
        (n_partition && !partition_channels) || (n_sort && (!sort_channels || !sort_desc))) {
        TG_SET_ERR("invalid topn_ranking spec: null argument or negative count");
        return TG_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n_partition; i++)
        if (partition_channels[i] < 0 || partition_channels[i] >= n_channels) {
            TG_SET_ERR("topn_ranking partition channel %d outside %d channels",
                       partition_channels[i], n_channels);
            return TG_ERR_INVALID_ARG;
        }
    for (int i = 0; i < n_sort; i++)
        if (sort_channels[i] < 0 || sort_channels[i] >= n_channels) {
            TG_SET_ERR("topn_ranking sort channel %d outside %d channels", sort_channels[i],
                       n_channels);
            return TG_ERR_INVALID_ARG;
        }
    if (ranking_fn < TG_RANKING_ROW_NUMBER || ranking_fn > TG_RANKING_DENSE_RANK) {
        TG_SET_ERR("topn_ranking: unknown ranking function %d", ranking_fn);
        return TG_ERR_INVALID_ARG;
    }
    if (max_ranking_per_partition < 1) {
        TG_SET_ERR("topn_ranking: max ranking %d, at least 1 required",
                   max_ranking_per_partition);
        return TG_ERR_INVALID_ARG;
    }
    if (emit_ranking < 0 || emit_ranking > 1) {
        TG_SET_ERR("topn_ranking: emit_ranking %d, 0 or 1 expected", emit_ranking);
        return TG_ERR_INVALID_ARG;
    }
    /* the payload gather moves fixed-width cells only (as TopN and Window) */
    for (int i = 0; i < n_channels; i++)
        if (types[i] == TG_VARCHAR) {
            TG_SET_ERR("topn_ranking: VARCHAR channel %d is not supported", i);
            return TG_ERR_UNSUPPORTED;
        }
    auto* op = new TopNRankingOp();
    op->s = s;
    for (int i = 0; i < n_channels; i++) op->types.push_back((tg_type)types[i]);
    op->partition_channels.assign(partition_channels, partition_channels + n_partition);
    op->sort_channels.assign(sort_channels, sort_channels + n_sort);
    op->sort_desc.assign(sort_desc, sort_desc + n_sort);
    op->fn = ranking_fn;
    op->limit = max_ranking_per_partition;
    op->emit_ranking = emit_ranking != 0;
    /* buffered rows that trigger a compaction; read here, once per operator.
     * MI355X, 2^24 rows of three BIGINT channels in 16 pages, ROW_NUMBER,
     * N = 10, median ms end to end (profiles/topn_ranking_cost.txt):
     *     threshold   ~2^20 partitions   one partition
     *     2^20             10.623            12.315
     *     2^22              9.150             5.829
     *     2^24              5.718             4.498
     * Every compaction is a sort of what is buffered, so the fewest
     * compactions win; the fastest of the three is kept. It is also the
     * memory bound: 2^24 rows of the input's channels stay buffered. */
    const char* e = getenv("TG_TOPNR_COMPACT_ROWS");
    int64_t rows = e ? atoll(e) : 0;
    op->threshold = rows >= 1 ? rows : ((int64_t)1 << 24);
    *out = op;
    return TG_OK;
}
