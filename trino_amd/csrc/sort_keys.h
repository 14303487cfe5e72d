/* sort_keys.h — the ordering path shared by the TopN operator (ops_topn.hip)
 * and the Window operator (ops_window.hip): the sortable image of a key cell,
 * and the declarations of the host functions in sort.hip that check an input
 * page, order the accumulated pages and gather them through an index array.
 * The kernels behind them are defined once, in sort.hip.
 */
#pragma once
#include "common.h"
#include "operators.h"
#include <utility>

/* order-preserving map to an unsigned "ascending sortable" key space:
 * integers: flip the sign bit; doubles: IEEE total-order trick after
 * canonicalising -0.0 to +0.0 and every NaN (either sign bit) to one quiet
 * NaN, so +-0 tie and all NaNs tie as the largest non-NULL value (Trino's
 * ORDER BY rule; TopN's host comparator agrees). DESC channels are stored
 * bit-inverted so every radix pass sorts ascending. NULLs are ordered by a
 * separate stable 1-bit pass (k_topn_null_keys): every u64 image belongs to
 * some value (INT64_MAX, NaN), so no in-band sentinel exists. */
__device__ static inline uint64_t topn_sortable(const void* data, int32_t type, int64_t i)
{
    const uint64_t SIGN = 0x8000000000000000ull;
    switch (type) {
        case TG_BIGINT: return (uint64_t)((const int64_t*)data)[i] ^ SIGN;
        case TG_INTEGER: case TG_DATE:
            return (uint64_t)(int64_t)((const int32_t*)data)[i] ^ SIGN;
        case TG_SMALLINT: return (uint64_t)(int64_t)((const int16_t*)data)[i] ^ SIGN;
        case TG_TINYINT: case TG_BOOLEAN:
            return (uint64_t)(int64_t)((const int8_t*)data)[i] ^ SIGN;
        default: {
            double v = ((const double*)data)[i];
            if (v != v) return 0x7FF8000000000000ull | SIGN;   /* one NaN */
            if (v == 0.0) v = 0.0;                               /* -0.0 -> +0.0 */
            long long b = __double_as_longlong(v);
            return b < 0 ? ~(uint64_t)b : ((uint64_t)b | SIGN);
        }
    }
}

/* key images of one ordering channel, indexed by flat input row */
struct SortKeyImages {
    const uint64_t* kf;   /* topn_sortable image, or a VARCHAR channel's rank (0 where NULL) */
    const uint64_t* nf;   /* null-pass bit; nullptr when the channel has no NULLs */
};

/* the page has at least types.size() channels, none VARCHAR, each as wide as
 * declared; `op` names the operator in the error text */
tg_status check_fixed_width_page(const char* op, const tg_page* page,
                                 const std::vector<tg_type>& types);

/* the same for operators that take VARCHAR: a VARCHAR block exactly where
 * `types` declares one, every other cell as wide as declared */
tg_status check_page(const char* op, const tg_page* page, const std::vector<tg_type>& types);

/* order the total_rows rows of `pages` by (channel, desc) keys, most
 * significant first, into d_perm[total_rows] (flat row indices; ASC = nulls
 * last, DESC = nulls first; whole-key ties keep input order). The image of a
 * VARCHAR key channel is the row's dense rank among the channel's non-NULL
 * strings in unsigned byte order (a proper prefix first), so
 * image equality is grouping equality for every type. Temporaries
 * come from `ps`; with `images` the per-key images are handed back, alive as
 * long as `ps`. */
tg_status order_pages(tg_session* s, PoolScratch& ps, const std::vector<DevPage>& pages,
                      int64_t total_rows,
                      const std::vector<std::pair<int32_t, int32_t>>& keys,
                      int64_t* d_perm, std::vector<SortKeyImages>* images);

/* gather channels [0, types.size()) of `pages`, or the channels listed in
 * out_channels (any subset, order or repetition), through the flat row
 * indices d_idx[take] into outp, validity included. A VARCHAR channel goes
 * through a lengths pass, a scan to offsets starting at 0 and a byte copy per
 * source page; a NULL VARCHAR cell has zero length. Asynchronous on the
 * session stream but for the one read of a VARCHAR channel's byte total; on
 * error outp holds what was allocated, for tg_free_page. */
tg_status gather_pages(tg_session* s, const std::vector<DevPage>& pages,
                       const std::vector<tg_type>& types, const int64_t* d_idx,
                       int64_t take, DevPage* outp,
                       const std::vector<int32_t>* out_channels = nullptr);
