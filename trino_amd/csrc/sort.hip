/* sort.hip — device ordering shared by the operators.
 *
 * Radix sorts: one rocPRIM recipe (sort_by_key) behind the run_sort_*
 * helpers, run_argsort_i64 (the group-by output remap of HashAggOp::emit) and
 * tg_dedup_i64. rocprim::radix_sort_pairs is stable, which the multi-key
 * ordering relies on (least-significant-key-first passes == lexicographic
 * order).
 *
 * The ordering path of TopN and Window (declared in sort_keys.h): the check
 * of an input page, order_pages (key images, then stable passes from an
 * iota) and gather_pages (every channel through an index array), with the
 * kernels they launch. Temporaries live in a PoolScratch, so every path
 * returns them to the session pool.
 */
#include "common.h"
#include "operators.h"
#include "sort_keys.h"
#include <rocprim/rocprim.hpp>
#include <type_traits>

__global__ void k_iota_i64(int64_t* v, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) v[i] = i;
}

__global__ void k_i64_to_i32(const int64_t* __restrict__ in, int64_t n,
                             int32_t* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = (int32_t)in[i];
}

struct NoValue {};

/* stable ascending radix sort over key bits [0, bits) of d_keys[n], with
 * d_vals[n] carried along unless V is NoValue; both updated in place
 * (sorted into a second buffer and copied back) */
template <typename K, typename V>
static tg_status sort_by_key(tg_session* s, K* d_keys, V* d_vals, int64_t n, int bits)
{
    constexpr bool pairs = !std::is_same<V, NoValue>::value;
    const char* what = pairs ? "radix_sort_pairs" : "radix_sort_keys";
    if (n <= 1) return TG_OK;
    PoolScratch ps(s);
    K* d_keys2 = nullptr;
    V* d_vals2 = nullptr;
    TG_TRY(ps.alloc(&d_keys2, n * sizeof(K)));
    if (pairs) TG_TRY(ps.alloc(&d_vals2, n * sizeof(V)));
    size_t temp_bytes = 0;
    auto sort = [&](void* d_temp) {
        if constexpr (pairs)
            return rocprim::radix_sort_pairs(d_temp, temp_bytes, d_keys, d_keys2, d_vals,
                                             d_vals2, (size_t)n, 0, bits, s->stream);
        else
            return rocprim::radix_sort_keys(d_temp, temp_bytes, d_keys, d_keys2, (size_t)n,
                                            0, bits, s->stream);
    };
    hipError_t e = sort(nullptr);
    if (e != hipSuccess) { TG_SET_ERR("rocprim size query: %s", hipGetErrorName(e)); return TG_ERR_HIP; }
    void* d_temp = nullptr;
    TG_TRY(ps.alloc(&d_temp, (int64_t)temp_bytes));
    e = sort(d_temp);
    if (e != hipSuccess) { TG_SET_ERR("rocprim %s: %s", what, hipGetErrorName(e)); return TG_ERR_HIP; }
    TG_HIP_CHECK(hipMemcpyAsync(d_keys, d_keys2, n * sizeof(K), hipMemcpyDeviceToDevice, s->stream));
    if (pairs)
        TG_HIP_CHECK(hipMemcpyAsync(d_vals, d_vals2, n * sizeof(V), hipMemcpyDeviceToDevice, s->stream));
    TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    return TG_OK;
}

/* (u64 key, i64 value) pairs. `bits` limits the radix passes when the key
 * range is known (e.g. pool offsets < 2^29). */
tg_status run_sort_pairs_bits(tg_session* s, uint64_t* d_keys, int64_t* d_vals,
                              int64_t n, int bits)
{
    return sort_by_key(s, d_keys, d_vals, n, bits);
}

tg_status run_sort_pairs(tg_session* s, uint64_t* d_keys, int64_t* d_vals, int64_t n)
{
    return sort_by_key(s, d_keys, d_vals, n, 64);
}

/* (u32 key, i32 value) pairs (join match reordering: sort matches by probe
 * row) */
tg_status run_sort_pairs_u32(tg_session* s, uint32_t* d_keys, int32_t* d_vals, int64_t n)
{
    return sort_by_key(s, d_keys, d_vals, n, 32);
}

/* keys-only u32 sort (segment-occurrence index for the indexed pool LIKE;
 * positions emitted by atomic append arrive unordered) */
tg_status run_sort_keys_u32(tg_session* s, uint32_t* d_keys, int64_t n)
{
    return sort_by_key(s, d_keys, (NoValue*)nullptr, n, 32);
}

/* argsort of non-negative i64 keys (ascending, stable): writes the
 * permutation as int32 into d_out_idx[n]. d_keys is clobbered. */
tg_status run_argsort_i64(tg_session* s, int64_t* d_keys, int64_t n, int32_t* d_out_idx)
{
    PoolScratch ps(s);
    int64_t* d_vals = nullptr;
    TG_TRY(ps.alloc(&d_vals, n * 8));
    hipLaunchKernelGGL(k_iota_i64, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0, s->stream,
                       d_vals, n);
    TG_HIP_CHECK(hipGetLastError());
    TG_TRY(run_sort_pairs(s, (uint64_t*)d_keys, d_vals, n));
    hipLaunchKernelGGL(k_i64_to_i32, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0, s->stream,
                       d_vals, n, d_out_idx);
    TG_HIP_CHECK(hipGetLastError());
    TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    return TG_OK;
}

/* sort-based DISTINCT of a non-negative BIGINT column: a keys-only radix sort
 * + rocprim::unique compaction, sequential-bandwidth only. Replaces the
 * generic hash aggregation dedup when nearly every row is unique (Q16's
 * ~12M distinct (combo,suppkey) pairs: the keystore insert + group-remap
 * sort pay random HBM round-trips per row; the sorted path streams).
 * d_out must hold n entries; *h_out_n gets the distinct count. `bits` is
 * the key width to sort (<=64; fewer radix passes for packed keys). */
extern "C" tg_status tg_dedup_i64(tg_session* s, const int64_t* d_in,
    int64_t n, int32_t bits, int64_t* d_out, int64_t* h_out_n)
{
    if (!s || !d_in || !d_out || !h_out_n || n < 0 || bits < 1 || bits > 64) {
        TG_SET_ERR("invalid dedup spec");
        return TG_ERR_INVALID_ARG;
    }
    if (n <= 1) {
        if (n == 1)
            TG_HIP_CHECK(hipMemcpyAsync(d_out, d_in, 8,
                                        hipMemcpyDeviceToDevice, s->stream));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        *h_out_n = n;
        return TG_OK;
    }
    PoolScratch ps(s);
    uint64_t* d_sorted = nullptr;
    int64_t* d_count = nullptr;
    TG_TRY(ps.alloc(&d_sorted, n * 8));
    TG_TRY(ps.alloc(&d_count, 8));
    TG_HIP_CHECK(hipMemcpyAsync(d_sorted, d_in, n * 8, hipMemcpyDeviceToDevice,
                                s->stream));
    TG_TRY(sort_by_key(s, d_sorted, (NoValue*)nullptr, n, bits));
    size_t u_bytes = 0;
    void* d_temp = nullptr;
    hipError_t e0 = rocprim::unique(nullptr, u_bytes, d_sorted, (uint64_t*)d_out,
                                    (int64_t*)d_count, (size_t)n,
                                    rocprim::equal_to<uint64_t>(), s->stream);
    if (e0 != hipSuccess) { TG_SET_ERR("rocprim unique size query: %s", hipGetErrorName(e0)); return TG_ERR_HIP; }
    TG_TRY(ps.alloc(&d_temp, (int64_t)u_bytes));
    hipError_t e = rocprim::unique(d_temp, u_bytes, d_sorted, (uint64_t*)d_out,
                                   (int64_t*)d_count, (size_t)n,
                                   rocprim::equal_to<uint64_t>(), s->stream);
    if (e != hipSuccess) { TG_SET_ERR("rocprim unique: %s", hipGetErrorName(e)); return TG_ERR_HIP; }
    TG_HIP_CHECK(hipMemcpyAsync(h_out_n, d_count, 8, hipMemcpyDeviceToHost,
                                s->stream));
    TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    return TG_OK;
}

/* ---- the ordering path of TopN and Window (sort_keys.h) ---- */

__global__ void k_topn_keys(const void* __restrict__ data,
                            const uint64_t* __restrict__ valid, int32_t type,
                            int32_t desc, int64_t n, uint64_t* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        bool isnull = valid && !((valid[i >> 6] >> (i & 63)) & 1);
        uint64_t key;
        if (isnull) key = 0ull;   /* placed by the null pass */
        else {
            key = topn_sortable(data, type, i);
            if (desc) key = ~key;
        }
        out[i] = key;
    }
}

/* 1-bit key of the null pass: ASC nulls last (1), DESC nulls first (0) */
__global__ void k_topn_null_keys(const uint64_t* __restrict__ valid, int32_t desc,
                                 int64_t n, uint64_t* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        bool isnull = valid && !((valid[i >> 6] >> (i & 63)) & 1);
        out[i] = (isnull != (desc != 0)) ? 1ull : 0ull;
    }
}

/* output gather of one source page: output slot o takes flat row idx[o] when
 * it lies in this page ([base, base + n)); a NULL source cell clears the
 * output's validity bit */
template <typename T>
__global__ void k_topn_gather(const T* __restrict__ src, const uint64_t* __restrict__ src_valid,
                              const int64_t* __restrict__ idx, int64_t take,
                              int64_t base, int64_t n, T* __restrict__ out,
                              uint64_t* __restrict__ out_valid)
{
    int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; o < take; o += stride) {
        int64_t r = idx[o] - base;
        if (r < 0 || r >= n) continue;
        out[o] = src[r];
        if (src_valid && !((src_valid[r >> 6] >> (r & 63)) & 1))
            atomicAnd((unsigned long long*)&out_valid[o >> 6], ~(1ull << (o & 63)));
    }
}

__global__ void k_gather_u64_by_perm(const uint64_t* __restrict__ kf,
                                     const int64_t* __restrict__ perm, int64_t n,
                                     uint64_t* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = kf[perm[i]];
}

tg_status check_fixed_width_page(const char* op, const tg_page* page,
                                 const std::vector<tg_type>& types)
{
    /* the output gather copies cells at the declared width */
    if (page->channel_count < (int32_t)types.size()) {
        TG_SET_ERR("%s page has %d channels, operator %zu", op, page->channel_count, types.size());
        return TG_ERR_INVALID_ARG;
    }
    for (size_t c = 0; c < types.size(); c++) {
        DevBlock want, got;
        want.type = types[c];
        got.type = (tg_type)page->blocks[c].type;
        if (got.type == TG_VARCHAR || got.elem_size() != want.elem_size()) {
            TG_SET_ERR("%s channel %zu type %d, operator declared %d", op, c,
                       page->blocks[c].type, (int)types[c]);
            return TG_ERR_INVALID_ARG;
        }
    }
    return TG_OK;
}

/* flat row index of each page's first row */
static std::vector<int64_t> page_bases(const std::vector<DevPage>& pages)
{
    std::vector<int64_t> base(pages.size() + 1, 0);
    for (size_t p = 0; p < pages.size(); p++) base[p + 1] = base[p] + pages[p].n;
    return base;
}

static bool channel_nullable(const std::vector<DevPage>& pages, size_t c)
{
    bool nullable = false;
    for (auto& pg : pages) nullable |= pg.n && pg.blocks[c].valid;
    return nullable;
}

/* per-channel sortable-u64 images, then stable radix passes least-significant
 * key first (lexicographic) starting from an iota */
tg_status order_pages(tg_session* s, PoolScratch& ps, const std::vector<DevPage>& pages,
                      int64_t total_rows,
                      const std::vector<std::pair<int32_t, int32_t>>& keys,
                      int64_t* d_perm, std::vector<SortKeyImages>* images)
{
    size_t k = keys.size();
    std::vector<int64_t> page_base = page_bases(pages);
    hipLaunchKernelGGL(k_iota_i64, dim3(tg_grid_for(total_rows)), dim3(TG_BLOCK),
                       0, s->stream, d_perm, total_rows);
    TG_HIP_CHECK(hipGetLastError());
    if (!k) return TG_OK;
    std::vector<uint64_t*> kf(k, nullptr), nf(k, nullptr);
    for (size_t j = 0; j < k; j++) {
        int32_t ch = keys[j].first, desc = keys[j].second;
        TG_TRY(ps.alloc(&kf[j], total_rows * 8));
        bool nullable = channel_nullable(pages, ch);
        if (nullable) TG_TRY(ps.alloc(&nf[j], total_rows * 8));
        for (size_t p = 0; p < pages.size(); p++) {
            const DevBlock& b = pages[p].blocks[ch];
            if (!pages[p].n) continue;
            hipLaunchKernelGGL(k_topn_keys, dim3(tg_grid_for(pages[p].n)),
                               dim3(TG_BLOCK), 0, s->stream, b.data, b.valid,
                               (int32_t)b.type, desc, pages[p].n,
                               kf[j] + page_base[p]);
            TG_HIP_CHECK(hipGetLastError());
            if (!nullable) continue;
            hipLaunchKernelGGL(k_topn_null_keys, dim3(tg_grid_for(pages[p].n)),
                               dim3(TG_BLOCK), 0, s->stream, b.valid,
                               desc, pages[p].n, nf[j] + page_base[p]);
            TG_HIP_CHECK(hipGetLastError());
        }
        if (images) images->push_back(SortKeyImages{kf[j], nf[j]});
    }
    uint64_t* d_keys = nullptr;
    TG_TRY(ps.alloc(&d_keys, total_rows * 8));
    for (int j = (int)k - 1; j >= 0; j--) {
        hipLaunchKernelGGL(k_gather_u64_by_perm, dim3(tg_grid_for(total_rows)),
                           dim3(TG_BLOCK), 0, s->stream, kf[j], d_perm,
                           total_rows, d_keys);
        TG_HIP_CHECK(hipGetLastError());
        TG_TRY(run_sort_pairs(s, d_keys, d_perm, total_rows));
        if (!nf[j]) continue;
        /* the channel's major order: NULL or not, one stable 1-bit pass */
        hipLaunchKernelGGL(k_gather_u64_by_perm, dim3(tg_grid_for(total_rows)),
                           dim3(TG_BLOCK), 0, s->stream, nf[j], d_perm,
                           total_rows, d_keys);
        TG_HIP_CHECK(hipGetLastError());
        TG_TRY(run_sort_pairs_bits(s, d_keys, d_perm, total_rows, 1));
    }
    return TG_OK;
}

/* one gather launch per (channel, source page): each output slot finds its
 * flat row in exactly one page; validity travels along */
tg_status gather_pages(tg_session* s, const std::vector<DevPage>& pages,
                       const std::vector<tg_type>& types, const int64_t* d_idx,
                       int64_t take, DevPage* outp)
{
    std::vector<int64_t> page_base = page_bases(pages);
    outp->n = take;
    for (size_t c = 0; c < types.size(); c++) {
        /* in the page before it owns anything: an error frees it with the page */
        outp->blocks.emplace_back();
        DevBlock& b = outp->blocks.back();
        b.type = types[c];
        b.n = take;
        TG_POOL_ALLOC(s, &b.data, (take ? take : 1) * b.elem_size());
        if (channel_nullable(pages, c)) {
            int64_t words = (take + 63) / 64;
            TG_POOL_ALLOC(s, &b.valid, (words ? words : 1) * 8);
            TG_HIP_CHECK(hipMemsetAsync(b.valid, 0xFF, words * 8, s->stream));
        }
        for (size_t p = 0; take && p < pages.size(); p++) {
            const DevBlock& sb = pages[p].blocks[c];
            int64_t pn = pages[p].n;
            if (!pn) continue;
            tg_dispatch_width(b.elem_size(), [&](auto t) {
                using T = decltype(t);
                hipLaunchKernelGGL(k_topn_gather<T>, dim3(tg_grid_for(take)), dim3(TG_BLOCK),
                                   0, s->stream, (const T*)sb.data, sb.valid, d_idx, take,
                                   page_base[p], pn, (T*)b.data, b.valid);
            });
            TG_HIP_CHECK(hipGetLastError());
        }
    }
    return TG_OK;
}
