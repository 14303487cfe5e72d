/* q1.hip — fused TPC-H Q1 scan+filter+aggregate kernel for gfx950.
 *
 * Replaces, in one HBM pass, the reference pipeline
 *   ScanFilterAndProjectOperator (ColumnarFilter shipdate<=cutoff,
 *   sql/gen/columnar/ColumnarFilter.java:42-52) ->
 *   projections extprice*(1-disc), *(1+tax) (project/PageProcessor.java:274-305) ->
 *   HashAggregationOperator over (returnflag, linestatus)
 *   (InMemoryHashAggregationBuilder.java:140-158, DoubleSumAggregation.java:37-45,
 *    DoubleAverageAggregations.java:38-63, CountAggregation).
 *
 * Algorithmic traffic: 38 B/row (shipdate i32 + 4 f64 + 2 u8); HBM-bound,
 * no MFMA (no dense contraction here). Roofline ceiling 8 TB/s / 38 B =
 * 210 Grow/s per GPU.
 *
 * FP sums are error-free fixed-point: every addend x has
 * ulp >= 2^-43 (money columns, x >= 2^9) or >= 2^-59 (discount), so
 * y = x * 2^scale is an exact u64 integer; lanes accumulate y into u128.
 * The final sums are the correctly-rounded exact sums, order-independent —
 * bit-equal to oracle o_q1_exact. sum(quantity) and count are exact integers.
 *
 * Structure of a step (two launches, no copy):
 *   k_q1_fused  one pass over the columns, 4 rows per lane per iteration.
 *     - The row loop is software-pipelined: the eleven loads (seven columns) of group
 *       i + stride are issued into a second register set before the ALU work
 *       on group i, so every wave keeps 152 B/lane in flight while it
 *       computes.
 *     - Per-lane sums are 96-bit and counts 32-bit (bounded by rows per
 *       lane, checked on the host) and widened at the wave reduce.
 *     - The six combo sections are guarded by one per-lane "combos present"
 *       bitmask, one wave vote per section.
 *     - Block partials go out word-major: partials[word][block].
 *   k_q1_merge  36 blocks, one per (combo, field); each reads its word's
 *     partials with unit stride, adds them as u128 and writes the final
 *     words straight into the session's pinned, device-mapped result block.
 *
 * Measured at SF100 on MI355X (profiles/q1_pipelined_vs_parent.txt): step
 * 4.19 -> 3.81 ms; scan 3.8 ms = 6.0 TB/s of the ~6.3 TB/s a streaming read
 * reaches; merge 4.6 us where the serial reduce + result copy took 0.14 ms.
 *
 * k_q1_fused_int is the same step over the exact integer forms of the four
 * numeric columns (13 B/row instead of 38): tg_q1_run launches it when the
 * column set carries all four (the generator fills them), k_q1_fused
 * otherwise; the 60 result words are identical. See "integer-column scan"
 * below and profiles/q1_int_columns_vs_parent.txt.
 *
 * Parity-mode kernel (k_q1_naive_seq): single thread, reference sequential
 * order — bit-equal to oracle o_q1_naive for page-sized operator tests.
 */
#include "common.h"
#include <cstdlib>

#define NCOMBO 6
#define S43 8796093022208.0        /* 2^43 */
#define S59 576460752303423488.0   /* 2^59 */
#define Q1_R 4                     /* rows per lane per iteration */

/* result layout: per combo 10 u64 words:
 * base(2) dp(2) ch(2) disc(2) qty(1) cnt(1) => 60 words.
 * partials are word-major: word w of block b is partials[w * TG_MAX_BLOCKS + b] */
#define PARTIAL_WORDS (NCOMBO * 10)

typedef double q1_f64x2 __attribute__((ext_vector_type(2)));
typedef int q1_i32x4 __attribute__((ext_vector_type(4)));

/* trunc(x * scale) as u64 for x >= 0, x * scale < 2^63 (scale a power of
 * two, so the product is exact) — the oracle's (long long)(x * S). An
 * integer-only version taken from the mantissa (seven 32-bit instructions
 * instead of seven f64 ones) was measured and showed no gain once the loop is
 * pipelined — the scan is HBM-bound — so the plain cast stays
 * (profiles/q1_pipelined_vs_parent.txt). */
__device__ static inline unsigned long long fx_trunc(double x, double scale)
{
    return (unsigned long long)(x * scale);
}

/* one lane's four rows of the seven columns (38 VGPRs) */
struct q1_rows {
    q1_f64x2 q[2], e[2], d[2], t[2];
    q1_i32x4 sd;
    unsigned rf, ls;   /* 4 packed bytes each */
};

/* the columns are read once and are 90x the Infinity Cache: nontemporal
 * loads (measured 4.14 -> 3.81 ms per SF100 step against plain loads) */
__device__ static inline void q1_load(q1_rows& g, int64_t r,
                                      const int32_t* __restrict__ shipdate,
                                      const double* __restrict__ qty,
                                      const double* __restrict__ extprice,
                                      const double* __restrict__ disc,
                                      const double* __restrict__ tax,
                                      const uint8_t* __restrict__ rflag,
                                      const uint8_t* __restrict__ lstatus)
{
    const q1_f64x2* pq = reinterpret_cast<const q1_f64x2*>(qty + r);
    const q1_f64x2* pe = reinterpret_cast<const q1_f64x2*>(extprice + r);
    const q1_f64x2* pd = reinterpret_cast<const q1_f64x2*>(disc + r);
    const q1_f64x2* pt = reinterpret_cast<const q1_f64x2*>(tax + r);
    g.q[0] = __builtin_nontemporal_load(pq); g.q[1] = __builtin_nontemporal_load(pq + 1);
    g.e[0] = __builtin_nontemporal_load(pe); g.e[1] = __builtin_nontemporal_load(pe + 1);
    g.d[0] = __builtin_nontemporal_load(pd); g.d[1] = __builtin_nontemporal_load(pd + 1);
    g.t[0] = __builtin_nontemporal_load(pt); g.t[1] = __builtin_nontemporal_load(pt + 1);
    g.sd = __builtin_nontemporal_load(reinterpret_cast<const q1_i32x4*>(shipdate + r));
    g.rf = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(rflag + r));
    g.ls = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(lstatus + r));
}

/* per-lane accumulators of one combo: the four u128 sums are kept as 96 bits
 * (a lane adds at most one carry per row into the top word, and the host
 * bounds rows per lane below 2^32), the count as 32 — 15 VGPRs per combo */
struct acc96 { unsigned w0, w1, w2; };
struct lane_acc {
    acc96 base, dp, ch, disc;
    unsigned long long qty;
    unsigned cnt;
};

/* three-instruction carry chain, in place */
__device__ static inline void acc_add(acc96& a, unsigned long long y)
{
    unsigned c0, c1;
    a.w0 = __builtin_addc(a.w0, (unsigned)y, 0u, &c0);
    a.w1 = __builtin_addc(a.w1, (unsigned)(y >> 32), c0, &c1);
    a.w2 += c1;
}

/* add one row's values to combo c; c must be a compile-time constant at
 * every call: a runtime acc[c] index demotes the
 * whole accumulator array to scratch (measured: 496 B/lane, 18% roofline) */
#define Q1_ACC_ADD(c, tb, tp, tc, td, tq, tn) do { \
    acc_add(acc[c].base, (tb)); \
    acc_add(acc[c].dp, (tp)); \
    acc_add(acc[c].ch, (tc)); \
    acc_add(acc[c].disc, (td)); \
    acc[c].qty += (tq); \
    acc[c].cnt += (tn); } while (0)

__device__ static inline void q1_accumulate(lane_acc (&acc)[NCOMBO], const q1_rows& g,
                                            int32_t cutoff)
{
    const double vq[Q1_R] = { g.q[0].x, g.q[0].y, g.q[1].x, g.q[1].y };
    const double ve[Q1_R] = { g.e[0].x, g.e[0].y, g.e[1].x, g.e[1].y };
    const double vd[Q1_R] = { g.d[0].x, g.d[0].y, g.d[1].x, g.d[1].y };
    const double vt[Q1_R] = { g.t[0].x, g.t[0].y, g.t[1].x, g.t[1].y };
    const int32_t sd[Q1_R] = { g.sd.x, g.sd.y, g.sd.z, g.sd.w };
    unsigned sc[Q1_R];      /* combo of a selected row, 0xffff otherwise */
    unsigned present = 0;   /* bit c: this lane has a selected row of combo c */
    unsigned long long yb[Q1_R], yp[Q1_R], yc[Q1_R], yd[Q1_R], yq[Q1_R];
    #pragma unroll
    for (int j = 0; j < Q1_R; j++) {
        const unsigned cb = ((g.rf >> (8 * j)) & 0xffu) * 2 + ((g.ls >> (8 * j)) & 0xffu);
        const bool sel = sd[j] <= cutoff;
        sc[j] = sel ? cb : 0xffffu;
        present |= sel ? (1u << (cb & 31u)) : 0u;
        const double dp = ve[j] * (1.0 - vd[j]);
        const double ch = dp * (1.0 + vt[j]);
        yb[j] = fx_trunc(ve[j], S43);
        yp[j] = fx_trunc(dp, S43);
        yc[j] = fx_trunc(ch, S43);
        yd[j] = fx_trunc(vd[j], S59);
        yq[j] = fx_trunc(vq[j], 1.0);
    }
    #pragma unroll
    for (int c = 0; c < NCOMBO; c++) {
        if (__any((int)(present & (1u << c)))) {
            /* rows are added in place under the lane mask: no selects, no
             * temporaries; every add is a three-word carry chain */
            #pragma unroll
            for (int j = 0; j < Q1_R; j++) {
                if (sc[j] == (unsigned)c)
                    Q1_ACC_ADD(c, yb[j], yp[j], yc[j], yd[j], yq[j], 1u);
            }
        }
    }
}

__device__ static inline void wave_reduce_u128(u128& v)
{
    #pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        unsigned long long lo = __shfl_xor(v.lo, off, 64);
        unsigned long long hi = __shfl_xor(v.hi, off, 64);
        unsigned long long nl = v.lo + lo;
        v.hi = v.hi + hi + (nl < lo);
        v.lo = nl;
    }
}

__device__ static inline void wave_reduce_u64(unsigned long long& v)
{
    #pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v += __shfl_xor(v, off, 64);
}

__global__ __launch_bounds__(TG_BLOCK, 2)   /* 2nd arg: waves/SIMD */
void k_q1_fused(int64_t n, const int32_t* __restrict__ shipdate,
                const double* __restrict__ qty, const double* __restrict__ extprice,
                const double* __restrict__ disc, const double* __restrict__ tax,
                const uint8_t* __restrict__ rflag, const uint8_t* __restrict__ lstatus,
                int32_t cutoff, unsigned long long* __restrict__ partials)
{
    lane_acc acc[NCOMBO];
    #pragma unroll
    for (int c = 0; c < NCOMBO; c++) {
        acc[c].base = acc[c].dp = acc[c].ch = acc[c].disc = acc96{0u, 0u, 0u};
        acc[c].qty = 0;
        acc[c].cnt = 0;
    }

    const int64_t stride = (int64_t)gridDim.x * blockDim.x;   /* lanes total */
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ngrp = n / Q1_R;

    /* software pipeline: `cur` holds group i, `nxt` receives group i + stride
     * while `cur` is computed on. The prefetch is unconditional in control
     * flow — a skipped load block would force every later wait to drain the
     * whole queue — so a lane's last iteration re-reads its own group i
     * (in bounds, discarded). No lane reads past row ngrp * 4 <= n. */
    if (gid < ngrp) {
        int64_t i = gid;
        q1_rows cur, nxt;
        q1_load(cur, Q1_R * i, shipdate, qty, extprice, disc, tax, rflag, lstatus);
        do {
            const int64_t in = i + stride;
            const int64_t ip = in < ngrp ? in : i;
            q1_load(nxt, Q1_R * ip, shipdate, qty, extprice, disc, tax, rflag, lstatus);
            q1_accumulate(acc, cur, cutoff);
            cur = nxt;
            i = in;
        } while (i < ngrp);
    }
    /* leftover rows [ngrp*4, n) handled by the first lane */
    for (int64_t r = ngrp * Q1_R; gid == 0 && r < n; r++) {
        if (shipdate[r] <= cutoff) {
            int ct = rflag[r] * 2 + lstatus[r];
            double dpv = extprice[r] * (1.0 - disc[r]);
            double chv = dpv * (1.0 + tax[r]);
            unsigned long long tb = fx_trunc(extprice[r], S43);
            unsigned long long tp = fx_trunc(dpv, S43);
            unsigned long long tc = fx_trunc(chv, S43);
            unsigned long long td = fx_trunc(disc[r], S59);
            unsigned long long tq = fx_trunc(qty[r], 1.0);
            #pragma unroll
            for (int c = 0; c < NCOMBO; c++) {
                if (ct == c) Q1_ACC_ADD(c, tb, tp, tc, td, tq, 1u);
            }
        }
    }

    /* wave -> block -> global reduction (integers: order-free, deterministic) */
    __shared__ unsigned long long lds[TG_BLOCK / 64][PARTIAL_WORDS];
    const int wave = threadIdx.x / 64;
    const int lane = threadIdx.x % 64;
    #pragma unroll
    for (int c = 0; c < NCOMBO; c++) {
        u128 b, p, h, d;
        #define Q1_WIDEN(v, a) do { v.lo = ((unsigned long long)(a).w1 << 32) | (a).w0; v.hi = (a).w2; } while (0)
        Q1_WIDEN(b, acc[c].base);
        Q1_WIDEN(p, acc[c].dp);
        Q1_WIDEN(h, acc[c].ch);
        Q1_WIDEN(d, acc[c].disc);
        #undef Q1_WIDEN
        unsigned long long q = acc[c].qty, k = acc[c].cnt;
        wave_reduce_u128(b);
        wave_reduce_u128(p);
        wave_reduce_u128(h);
        wave_reduce_u128(d);
        wave_reduce_u64(q);
        wave_reduce_u64(k);
        if (lane == 0) {
            unsigned long long* w = lds[wave] + c * 10;
            w[0] = b.lo; w[1] = b.hi;
            w[2] = p.lo; w[3] = p.hi;
            w[4] = h.lo; w[5] = h.hi;
            w[6] = d.lo; w[7] = d.hi;
            w[8] = q;    w[9] = k;
        }
    }
    __syncthreads();
    if (threadIdx.x < PARTIAL_WORDS) {
        const int f = threadIdx.x;          /* one word per thread */
        const int is_hi = ((f % 10) < 8) && (f % 2 == 1);
        unsigned long long* pw = partials + (int64_t)f * TG_MAX_BLOCKS + blockIdx.x;
        if (!is_hi && (f % 10) < 8) {
            /* lo word of a u128 field: sum los, carries go into the hi word */
            unsigned long long lo = 0, hisum = 0;
            #pragma unroll
            for (int w = 0; w < TG_BLOCK / 64; w++) {
                unsigned long long x = lds[w][f];
                lo += x;
                hisum += (lo < x);
            }
            #pragma unroll
            for (int w = 0; w < TG_BLOCK / 64; w++) hisum += lds[w][f + 1];
            pw[0] = lo;
            pw[TG_MAX_BLOCKS] = hisum;
        }
        else if ((f % 10) >= 8) {
            unsigned long long s = 0;
            #pragma unroll
            for (int w = 0; w < TG_BLOCK / 64; w++) s += lds[w][f];
            pw[0] = s;
        }
        /* hi words written by their lo-word thread */
    }
}

/* ---- integer-column scan ------------------------------------------------
 * The same sums from the exact integer forms of the four numeric columns
 * (tg_tpch_lineitem_cols: quantity_u8, extendedprice_cents, discount_pct,
 * tax_pct): 13 B/row instead of 38. Every row's doubles are rebuilt bit for
 * bit — e = cents/100.0, d = pct/100.0, t = pct/100.0 — and then go through
 * exactly k_q1_fused's arithmetic, so the 60 result words are identical.
 *
 *   price       cents/100.0 without a divide: q0 = k*0.01, r = fma(-q0,100,k),
 *               q = fma(r,0.01,q0) equals the IEEE quotient for every k in
 *               [0, 2^31) (checked exhaustively on the host); plain k*0.01 is
 *               wrong for 288,120,706 of them.
 *   percentages a byte has 256 values: each block builds, with the f64 path's
 *               own expressions, LDS tables of 1.0-d and trunc(d*2^59) by
 *               discount byte and 1.0+t by tax byte; a row costs one
 *               ds_read_b128 and one ds_read_b64 instead of two decodes, two
 *               adds and one f64->u64 conversion.
 *   quantity    the byte is the integer addend; no f64 at all.
 *
 * A lane takes Q1I_R rows per iteration (one or more dwordx4 of price and
 * shipdate, Q1I_R/4 dwords of each byte column: every load is >= 4 B per lane
 * and coalesced) and works through them four at a time with k_q1_fused's
 * section scheme. Pipelining, nontemporal loads, compile-time combo indices,
 * 96-bit sums and 32-bit counts are as in k_q1_fused.
 *
 * Measured at SF100 (profiles/q1_int_columns_vs_parent.txt):
 * the scan is issue-bound, not HBM-bound. Q1I_R = 4 needs 166 VGPRs and runs
 * 3 waves/SIMD, which beats 8 and 16 rows per lane at 2 waves/SIMD; the fma
 * decode beats the divide; carry-free split sums (no s_nop hazard slots) and
 * a bit-level trunc were built, verified and measured no gain at Q1I_R = 4. */
#ifndef Q1I_R
#define Q1I_R 4                    /* rows per lane per iteration: 4, 8 or 16 */
#endif
#define Q1I_GRID_CAP 1536          /* blocks; TG_Q1_BLOCKS overrides */
#define Q1I_W (Q1I_R / 4)          /* dwords per byte column, dwordx4 per i32 column */
static_assert(Q1I_R == 4 || Q1I_R == 8 || Q1I_R == 16, "Q1I_R: whole dwordx4 groups");

struct q1i_rows {
    q1_i32x4 pc[Q1I_W], sd[Q1I_W];
    unsigned q[Q1I_W], d[Q1I_W], t[Q1I_W], rf[Q1I_W], ls[Q1I_W];   /* 4 packed bytes each */
};

/* Q1I_W consecutive dwords of a byte column as one load */
__device__ static inline void q1i_load_bytes(unsigned (&w)[Q1I_W], const uint8_t* __restrict__ p)
{
#if Q1I_W == 1
    w[0] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(p));
#else
    typedef unsigned wvec __attribute__((ext_vector_type(Q1I_W)));
    const wvec v = __builtin_nontemporal_load(reinterpret_cast<const wvec*>(p));
    #pragma unroll
    for (int k = 0; k < Q1I_W; k++) w[k] = v[k];
#endif
}

__device__ static inline void q1i_load(q1i_rows& g, int64_t r,
                                       const int32_t* __restrict__ shipdate,
                                       const int32_t* __restrict__ cents,
                                       const uint8_t* __restrict__ qty,
                                       const uint8_t* __restrict__ disc,
                                       const uint8_t* __restrict__ tax,
                                       const uint8_t* __restrict__ rflag,
                                       const uint8_t* __restrict__ lstatus)
{
    const q1_i32x4* pp = reinterpret_cast<const q1_i32x4*>(cents + r);
    const q1_i32x4* ps = reinterpret_cast<const q1_i32x4*>(shipdate + r);
    #pragma unroll
    for (int k = 0; k < Q1I_W; k++) {
        g.pc[k] = __builtin_nontemporal_load(pp + k);
        g.sd[k] = __builtin_nontemporal_load(ps + k);
    }
    q1i_load_bytes(g.q, qty + r);
    q1i_load_bytes(g.d, disc + r);
    q1i_load_bytes(g.t, tax + r);
    q1i_load_bytes(g.rf, rflag + r);
    q1i_load_bytes(g.ls, lstatus + r);
}

/* (double)k / 100.0 for 0 <= k < 2^31, bit for bit, without the divide */
__device__ static inline double q1i_cents_to_double(int32_t k)
{
    const double kd = (double)k;
    const double q0 = kd * 0.01;
    const double r = __fma_rn(-q0, 100.0, kd);
    return __fma_rn(r, 0.01, q0);
}

/* per-block decode tables, indexed by the column byte */
struct q1i_tables {
    ulonglong2 d[256];   /* .x = bits of 1.0 - d, .y = trunc(d * 2^59) */
    double opt[256];     /* 1.0 + t */
};

__device__ static inline void q1i_build_tables(q1i_tables& tab)
{
    static_assert(TG_BLOCK == 256, "one table entry per thread");
    const double v = (double)threadIdx.x / 100.0;   /* the generator's expression */
    tab.d[threadIdx.x].x = (unsigned long long)__double_as_longlong(1.0 - v);
    tab.d[threadIdx.x].y = fx_trunc(v, S59);
    tab.opt[threadIdx.x] = 1.0 + v;
    __syncthreads();
}

/* one row's five addends from its integers */
__device__ static inline void q1i_row(const q1i_tables& tab, int32_t cents, unsigned dpct,
                                      unsigned tpct, unsigned long long& yb,
                                      unsigned long long& yp, unsigned long long& yc,
                                      unsigned long long& yd)
{
    const double e = q1i_cents_to_double(cents);
    const ulonglong2 dd = tab.d[dpct];
    const double dp = e * __longlong_as_double((long long)dd.x);
    const double ch = dp * tab.opt[tpct];
    yb = fx_trunc(e, S43);
    yp = fx_trunc(dp, S43);
    yc = fx_trunc(ch, S43);
    yd = dd.y;
}

/* four rows (one dword of each byte column) into the lane's accumulators */
__device__ static inline void q1i_accumulate4(lane_acc (&acc)[NCOMBO], const q1i_tables& tab,
                                              q1_i32x4 pc, q1_i32x4 sdv, unsigned qw,
                                              unsigned dw, unsigned tw, unsigned rfw,
                                              unsigned lsw, int32_t cutoff)
{
    const int32_t ce[4] = { pc.x, pc.y, pc.z, pc.w };
    const int32_t sd[4] = { sdv.x, sdv.y, sdv.z, sdv.w };
    unsigned sc[4];         /* combo of a selected row, 0xffff otherwise */
    unsigned present = 0;   /* bit c: this lane has a selected row of combo c */
    unsigned long long yb[4], yp[4], yc[4], yd[4];
    unsigned yq[4];
    #pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned cb = ((rfw >> (8 * j)) & 0xffu) * 2 + ((lsw >> (8 * j)) & 0xffu);
        const bool sel = sd[j] <= cutoff;
        sc[j] = sel ? cb : 0xffffu;
        present |= sel ? (1u << (cb & 31u)) : 0u;
        q1i_row(tab, ce[j], (dw >> (8 * j)) & 0xffu, (tw >> (8 * j)) & 0xffu,
                yb[j], yp[j], yc[j], yd[j]);
        yq[j] = (qw >> (8 * j)) & 0xffu;
    }
    #pragma unroll
    for (int c = 0; c < NCOMBO; c++) {
        if (__any((int)(present & (1u << c)))) {
            #pragma unroll
            for (int j = 0; j < 4; j++) {
                if (sc[j] == (unsigned)c)
                    Q1_ACC_ADD(c, yb[j], yp[j], yc[j], yd[j], yq[j], 1u);
            }
        }
    }
}

/* wave -> block reduction of the lane accumulators and the block's word-major
 * partials (integers: order-free, deterministic); k_q1_fused's epilogue */
__device__ static inline void q1_block_reduce(const lane_acc (&acc)[NCOMBO],
                                              unsigned long long (&lds)[TG_BLOCK / 64][PARTIAL_WORDS],
                                              unsigned long long* __restrict__ partials)
{
    const int wave = threadIdx.x / 64;
    const int lane = threadIdx.x % 64;
    #pragma unroll
    for (int c = 0; c < NCOMBO; c++) {
        u128 b, p, h, d;
        #define Q1_WIDEN(v, a) do { v.lo = ((unsigned long long)(a).w1 << 32) | (a).w0; v.hi = (a).w2; } while (0)
        Q1_WIDEN(b, acc[c].base);
        Q1_WIDEN(p, acc[c].dp);
        Q1_WIDEN(h, acc[c].ch);
        Q1_WIDEN(d, acc[c].disc);
        #undef Q1_WIDEN
        unsigned long long q = acc[c].qty, k = acc[c].cnt;
        wave_reduce_u128(b);
        wave_reduce_u128(p);
        wave_reduce_u128(h);
        wave_reduce_u128(d);
        wave_reduce_u64(q);
        wave_reduce_u64(k);
        if (lane == 0) {
            unsigned long long* w = lds[wave] + c * 10;
            w[0] = b.lo; w[1] = b.hi;
            w[2] = p.lo; w[3] = p.hi;
            w[4] = h.lo; w[5] = h.hi;
            w[6] = d.lo; w[7] = d.hi;
            w[8] = q;    w[9] = k;
        }
    }
    __syncthreads();
    if (threadIdx.x < PARTIAL_WORDS) {
        const int f = threadIdx.x;          /* one word per thread */
        unsigned long long* pw = partials + (int64_t)f * TG_MAX_BLOCKS + blockIdx.x;
        if ((f % 10) < 8 && f % 2 == 0) {
            /* lo word of a u128 field: sum los, carries go into the hi word,
             * which this thread writes too */
            unsigned long long lo = 0, hisum = 0;
            #pragma unroll
            for (int w = 0; w < TG_BLOCK / 64; w++) {
                unsigned long long x = lds[w][f];
                lo += x;
                hisum += (lo < x);
            }
            #pragma unroll
            for (int w = 0; w < TG_BLOCK / 64; w++) hisum += lds[w][f + 1];
            pw[0] = lo;
            pw[TG_MAX_BLOCKS] = hisum;
        }
        else if ((f % 10) >= 8) {
            unsigned long long s = 0;
            #pragma unroll
            for (int w = 0; w < TG_BLOCK / 64; w++) s += lds[w][f];
            pw[0] = s;
        }
    }
}

__global__ __launch_bounds__(TG_BLOCK, 2)   /* 2nd arg: waves/SIMD, at least */
void k_q1_fused_int(int64_t n, const int32_t* __restrict__ shipdate,
                    const uint8_t* __restrict__ qty, const int32_t* __restrict__ cents,
                    const uint8_t* __restrict__ disc, const uint8_t* __restrict__ tax,
                    const uint8_t* __restrict__ rflag, const uint8_t* __restrict__ lstatus,
                    int32_t cutoff, unsigned long long* __restrict__ partials)
{
    __shared__ q1i_tables tab;
    __shared__ unsigned long long lds[TG_BLOCK / 64][PARTIAL_WORDS];
    q1i_build_tables(tab);

    lane_acc acc[NCOMBO];
    #pragma unroll
    for (int c = 0; c < NCOMBO; c++) {
        acc[c].base = acc[c].dp = acc[c].ch = acc[c].disc = acc96{0u, 0u, 0u};
        acc[c].qty = 0;
        acc[c].cnt = 0;
    }

    const int64_t stride = (int64_t)gridDim.x * blockDim.x;   /* lanes total */
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ngrp = n / Q1I_R;

    /* the pipeline of k_q1_fused: `nxt` receives group i + stride while `cur`
     * is computed on; a lane's last iteration re-reads its own group (in
     * bounds, discarded). No lane reads past row ngrp * Q1I_R <= n. */
    if (gid < ngrp) {
        int64_t i = gid;
        q1i_rows cur, nxt;
        q1i_load(cur, Q1I_R * i, shipdate, cents, qty, disc, tax, rflag, lstatus);
        do {
            const int64_t in = i + stride;
            const int64_t ip = in < ngrp ? in : i;
            q1i_load(nxt, Q1I_R * ip, shipdate, cents, qty, disc, tax, rflag, lstatus);
            #pragma unroll
            for (int k = 0; k < Q1I_W; k++)
                q1i_accumulate4(acc, tab, cur.pc[k], cur.sd[k], cur.q[k], cur.d[k],
                                cur.t[k], cur.rf[k], cur.ls[k], cutoff);
            cur = nxt;
            i = in;
        } while (i < ngrp);
    }
    /* leftover rows [ngrp * Q1I_R, n) handled by the first lane */
    for (int64_t r = ngrp * Q1I_R; gid == 0 && r < n; r++) {
        if (shipdate[r] <= cutoff) {
            const int ct = rflag[r] * 2 + lstatus[r];
            unsigned long long tb, tp, tc, td;
            q1i_row(tab, cents[r], disc[r], tax[r], tb, tp, tc, td);
            const unsigned tq = qty[r];
            #pragma unroll
            for (int c = 0; c < NCOMBO; c++) {
                if (ct == c) Q1_ACC_ADD(c, tb, tp, tc, td, tq, 1u);
            }
        }
    }
    q1_block_reduce(acc, lds, partials);
}

/* final cross-block merge: block (c, f) owns field f of combo c (f < 4: a
 * u128 sum, f = 4 qty, f = 5 count) and reads that word's partials with unit
 * stride across blocks. `out` is the session's device-mapped pinned block. */
#define MERGE_FIELDS 6
__global__ __launch_bounds__(TG_BLOCK)
void k_q1_merge(const unsigned long long* __restrict__ partials, int nblocks,
                unsigned long long* __restrict__ out)
{
    const int c = blockIdx.x / MERGE_FIELDS, f = blockIdx.x % MERGE_FIELDS;
    const int word = c * 10 + (f < 4 ? 2 * f : 8 + (f - 4));
    const unsigned long long* plo = partials + (int64_t)word * TG_MAX_BLOCKS;
    const unsigned long long* phi = plo + TG_MAX_BLOCKS;
    u128 s;
    for (int b = threadIdx.x; b < nblocks; b += TG_BLOCK) {
        u128 v;
        v.lo = plo[b];
        v.hi = f < 4 ? phi[b] : 0ull;
        s.add128(v);
    }
    wave_reduce_u128(s);
    __shared__ unsigned long long wl[TG_BLOCK / 64], wh[TG_BLOCK / 64];
    if (threadIdx.x % 64 == 0) {
        wl[threadIdx.x / 64] = s.lo;
        wh[threadIdx.x / 64] = s.hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u128 t;
        #pragma unroll
        for (int w = 0; w < TG_BLOCK / 64; w++) {
            u128 v; v.lo = wl[w]; v.hi = wh[w];
            t.add128(v);
        }
        out[word] = t.lo;
        if (f < 4) out[word + 1] = t.hi;
    }
}

/* parity-mode: the reference's single-driver sequential accumulation order
 * (bit-equal to oracle o_q1_naive). One thread; page-sized inputs only. */
__global__ void k_q1_naive_seq(int64_t n, const int32_t* shipdate, const double* qty,
                               const double* extprice, const double* disc,
                               const double* tax, const uint8_t* rflag,
                               const uint8_t* lstatus, int32_t cutoff,
                               double* sums /* [6][5]: qty,base,dp,ch,disc */,
                               long long* cnts /* [6] */)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int c = 0; c < NCOMBO; c++) {
        for (int f = 0; f < 5; f++) sums[c * 5 + f] = 0.0;
        cnts[c] = 0;
    }
    for (int64_t i = 0; i < n; i++) {
        if (shipdate[i] > cutoff) continue;
        int c = rflag[i] * 2 + lstatus[i];
        double dp = extprice[i] * (1.0 - disc[i]);
        double ch = dp * (1.0 + tax[i]);
        sums[c * 5 + 0] += qty[i];
        sums[c * 5 + 1] += extprice[i];
        sums[c * 5 + 2] += dp;
        sums[c * 5 + 3] += ch;
        sums[c * 5 + 4] += disc[i];
        cnts[c]++;
    }
}

/* the session owns Q1's working set; tg_session_close frees it */
static tg_status q1_ensure_scratch(tg_session* s)
{
    if (!s->q1_partials)
        TG_HIP_CHECK(hipMalloc(&s->q1_partials, (size_t)TG_MAX_BLOCKS * PARTIAL_WORDS * 8));
    if (!s->q1_result_dev) {
        if (!s->q1_result)
            TG_HIP_CHECK(hipHostMalloc((void**)&s->q1_result, PARTIAL_WORDS * 8, hipHostMallocMapped));
        TG_HIP_CHECK(hipHostGetDevicePointer((void**)&s->q1_result_dev, s->q1_result, 0));
    }
    if (!s->q1_naive_sums)
        TG_HIP_CHECK(hipMalloc(&s->q1_naive_sums, NCOMBO * 5 * 8));
    if (!s->q1_naive_cnts)
        TG_HIP_CHECK(hipMalloc(&s->q1_naive_cnts, NCOMBO * 8));
    return TG_OK;
}

void tg_q1_scratch_free(tg_session* s)
{
    if (s->q1_partials) (void)hipFree(s->q1_partials);
    if (s->q1_result) (void)hipHostFree(s->q1_result);
    if (s->q1_naive_sums) (void)hipFree(s->q1_naive_sums);
    if (s->q1_naive_cnts) (void)hipFree(s->q1_naive_cnts);
    s->q1_partials = s->q1_result = s->q1_result_dev = nullptr;
    s->q1_naive_sums = nullptr;
    s->q1_naive_cnts = nullptr;
}

extern "C" tg_status tg_q1_run(tg_session* s, const tg_tpch_lineitem_cols* cols,
                               int32_t cutoff, tg_q1_result* out)
{
    if (!s || !cols || !out) { TG_SET_ERR("null arg"); return TG_ERR_INVALID_ARG; }
    tg_status st = q1_ensure_scratch(s);
    if (st != TG_OK) return st;
    int64_t n = cols->row_count;
    /* grid sweep hook (default measured on MI355X; profiles/q1_pipelined_vs_parent.txt) */
    static int blocks_env = [] { const char* e = getenv("TG_Q1_BLOCKS"); return e ? atoi(e) : 0; }();
    /* the integer forms are all set or none is (trino_gpu.h); anything else
     * reads the f64 columns */
    const bool ints = cols->quantity_u8 && cols->extendedprice_cents &&
                      cols->discount_pct && cols->tax_pct;
    int grid = tg_grid_for(n, ints ? Q1I_R : Q1_R);
    const int cap = ints ? Q1I_GRID_CAP : 1536;
    if (grid > cap) grid = cap;
    if (blocks_env > 0) grid = blocks_env;
    if (grid > TG_MAX_BLOCKS) grid = TG_MAX_BLOCKS;   /* partials buffer bound */
    /* the per-lane carry words and counts are 32-bit */
    if (n / ((int64_t)grid * TG_BLOCK) >= 0xfffffff0ll) {
        TG_SET_ERR("q1: %lld rows exceed the per-lane 32-bit row bound", (long long)n);
        return TG_ERR_INVALID_ARG;
    }
    TG_HIP_CHECK(hipEventRecord(s->ev_start, s->stream));
    if (ints)
        hipLaunchKernelGGL(k_q1_fused_int, dim3(grid), dim3(TG_BLOCK), 0, s->stream,
                           n, cols->shipdate, cols->quantity_u8, cols->extendedprice_cents,
                           cols->discount_pct, cols->tax_pct, cols->returnflag,
                           cols->linestatus, cutoff, s->q1_partials);
    else
        hipLaunchKernelGGL(k_q1_fused, dim3(grid), dim3(TG_BLOCK), 0, s->stream,
                           n, cols->shipdate, cols->quantity, cols->extendedprice,
                           cols->discount, cols->tax, cols->returnflag, cols->linestatus,
                           cutoff, s->q1_partials);
    TG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_q1_merge, dim3(NCOMBO * MERGE_FIELDS), dim3(TG_BLOCK), 0, s->stream,
                       s->q1_partials, grid, s->q1_result_dev);
    TG_HIP_CHECK(hipGetLastError());
    /* the events bracket the scan and its merge */
    TG_HIP_CHECK(hipEventRecord(s->ev_stop, s->stream));
    TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    float ms = 0;
    TG_HIP_CHECK(hipEventElapsedTime(&ms, s->ev_start, s->ev_stop));

    unsigned long long h[PARTIAL_WORDS];
    memcpy(h, s->q1_result, sizeof(h));
    memset(out, 0, sizeof(*out));
    memcpy(out->raw, h, sizeof(h));
    for (int c = 0; c < NCOMBO; c++) {
        const unsigned long long* w = h + c * 10;
        __int128 base = ((__int128)w[1] << 64) | w[0];
        __int128 dp   = ((__int128)w[3] << 64) | w[2];
        __int128 ch   = ((__int128)w[5] << 64) | w[4];
        __int128 dc   = ((__int128)w[7] << 64) | w[6];
        out->sum_base[c] = (double)base / S43;
        out->sum_disc_price[c] = (double)dp / S43;
        out->sum_charge[c] = (double)ch / S43;
        out->sum_disc[c] = (double)dc / S59;
        out->sum_qty[c] = (double)(long long)w[8];
        out->count[c] = (int64_t)w[9];
        if (out->count[c] > 0) {
            out->avg_qty[c] = out->sum_qty[c] / (double)out->count[c];
            out->avg_price[c] = out->sum_base[c] / (double)out->count[c];
            out->avg_disc[c] = out->sum_disc[c] / (double)out->count[c];
        }
    }
    out->elapsed_ms = (double)ms;
    return TG_OK;
}

/* parity-mode entry (naive sequential; page-sized inputs) */
extern "C" tg_status tg_q1_run_naive(tg_session* s, const tg_tpch_lineitem_cols* cols,
                                     int32_t cutoff, tg_q1_result* out)
{
    if (!s || !cols || !out) { TG_SET_ERR("null arg"); return TG_ERR_INVALID_ARG; }
    tg_status st = q1_ensure_scratch(s);
    if (st != TG_OK) return st;
    hipLaunchKernelGGL(k_q1_naive_seq, dim3(1), dim3(64), 0, s->stream,
                       cols->row_count, cols->shipdate, cols->quantity,
                       cols->extendedprice, cols->discount, cols->tax,
                       cols->returnflag, cols->linestatus, cutoff,
                       s->q1_naive_sums, s->q1_naive_cnts);
    TG_HIP_CHECK(hipGetLastError());
    double hs[NCOMBO * 5];
    long long hc[NCOMBO];
    TG_HIP_CHECK(hipMemcpyAsync(hs, s->q1_naive_sums, sizeof(hs), hipMemcpyDeviceToHost, s->stream));
    TG_HIP_CHECK(hipMemcpyAsync(hc, s->q1_naive_cnts, sizeof(hc), hipMemcpyDeviceToHost, s->stream));
    TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    memset(out, 0, sizeof(*out));
    for (int c = 0; c < NCOMBO; c++) {
        out->sum_qty[c] = hs[c * 5 + 0];
        out->sum_base[c] = hs[c * 5 + 1];
        out->sum_disc_price[c] = hs[c * 5 + 2];
        out->sum_charge[c] = hs[c * 5 + 3];
        out->sum_disc[c] = hs[c * 5 + 4];
        out->count[c] = hc[c];
        if (hc[c] > 0) {
            out->avg_qty[c] = out->sum_qty[c] / (double)hc[c];
            out->avg_price[c] = out->sum_base[c] / (double)hc[c];
            out->avg_disc[c] = out->sum_disc[c] / (double)hc[c];
        }
    }
    return TG_OK;
}
