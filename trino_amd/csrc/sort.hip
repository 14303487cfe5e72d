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
#include "var_keys.h"
#include <rocprim/rocprim.hpp>
#include <cstdlib>
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

tg_status check_page(const char* op, const tg_page* page, const std::vector<tg_type>& types)
{
    if (page->channel_count < (int32_t)types.size()) {
        TG_SET_ERR("%s page has %d channels, operator %zu", op, page->channel_count, types.size());
        return TG_ERR_INVALID_ARG;
    }
    for (size_t c = 0; c < types.size(); c++) {
        DevBlock want, got;
        want.type = types[c];
        got.type = (tg_type)page->blocks[c].type;
        /* a VARCHAR block exactly where one was declared; cells as wide as
         * declared everywhere else */
        if ((got.type == TG_VARCHAR) != (want.type == TG_VARCHAR) ||
            (want.type != TG_VARCHAR && got.elem_size() != want.elem_size())) {
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

/* ---- the image of a VARCHAR key channel: dense ranks by chunk refinement
 * (DESIGN.md §6k). Every launch is elementwise or a scan; the host reads two
 * ints per round. ---- */

/* per (channel, page): the length of every row (0 where NULL) at its flat
 * position, and whether the channel holds a NULL / a non-NULL '' at all.
 * seen[0] / seen[1] only ever receive the value 1. */
__global__ void k_var_lens(const int32_t* __restrict__ off,
                           const uint64_t* __restrict__ valid, int64_t n,
                           int32_t* __restrict__ len, int32_t* __restrict__ seen)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        bool isnull = valid && !((valid[i >> 6] >> (i & 63)) & 1);
        int32_t l = isnull ? 0 : off[i + 1] - off[i];
        len[i] = l;
        if (isnull) seen[0] = 1;
        else if (l == 0) seen[1] = 1;
    }
}

/* per (channel, page): the round's chunk of every row at its flat position.
 * `len` is the page's slice of the flat lengths, so a NULL row reads nothing */
__global__ void k_var_chunks(const uint8_t* __restrict__ bytes,
                             const int32_t* __restrict__ off,
                             const int32_t* __restrict__ len, int64_t n, int32_t round,
                             uint64_t* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = varchar_chunk(bytes + off[i], len[i], round);
}

/* the length round's image */
__global__ void k_var_len_image(const int32_t* __restrict__ len, int64_t n,
                                uint64_t* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = (uint64_t)len[i];
}

/* positions are in (rank, image) order. a[i] = 1 where position i starts a
 * new (rank, image) group, a[0] = a[n] = 0: the exclusive scan of a[n + 1]
 * leaves the new dense rank of position i in a[i + 1]. *more is set where a
 * position ties with the one before it and either string goes on past
 * `seen_bytes`, the bytes compared so far. */
__global__ void k_var_flags(const int64_t* __restrict__ perm,
                            const uint64_t* __restrict__ rank,
                            const uint64_t* __restrict__ image,
                            const int32_t* __restrict__ len, int64_t n,
                            int64_t seen_bytes, int32_t* __restrict__ a,
                            int32_t* __restrict__ more)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        if (i == 0) { a[0] = 0; a[n] = 0; continue; }
        int64_t row = perm[i], prev = perm[i - 1];
        bool differs = rank[row] != rank[prev] || image[row] != image[prev];
        a[i] = differs ? 1 : 0;
        if (!differs && ((int64_t)len[row] > seen_bytes || (int64_t)len[prev] > seen_bytes))
            *more = 1;
    }
}

__global__ void k_var_scatter_ranks(const int64_t* __restrict__ perm,
                                    const int32_t* __restrict__ a, int64_t n,
                                    uint64_t* __restrict__ rank)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) rank[perm[i]] = (uint64_t)(uint32_t)a[i + 1];
}

/* per (channel, page): ranks to the image order_pages sorts. NULL rows took
 * part in the refinement as '' (length 0), so when the channel has NULLs but
 * no '' the ranks of the strings start at 1: shift them down, then they are
 * 0-based dense ranks among the non-NULL strings either way. */
__global__ void k_var_finish(const uint64_t* __restrict__ valid, int32_t desc, int64_t n,
                             const int32_t* __restrict__ seen, uint64_t* __restrict__ kf)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t shift = (seen[0] && !seen[1]) ? 1 : 0;
    for (; i < n; i += stride) {
        bool isnull = valid && !((valid[i >> 6] >> (i & 63)) & 1);
        uint64_t key = 0ull;   /* placed by the null pass */
        if (!isnull) {
            key = kf[i] - shift;
            if (desc) key = ~key;
        }
        kf[i] = key;
    }
}

/* one refinement round over `image` (chunks, or lengths): stable sort by
 * image, then by the current rank, flags, scan, scatter. d_state[0] = more,
 * d_state[1] = new groups found (rank count - 1), read back into h_state. */
static tg_status var_refine_round(tg_session* s, int64_t n, const uint64_t* d_image,
                                  const int32_t* d_len, int64_t seen_bytes, int rank_bits,
                                  uint64_t* d_rank, int64_t* d_perm, uint64_t* d_keys,
                                  int32_t* d_a, int32_t* d_state, int32_t* h_state)
{
    int grid = tg_grid_for(n);
    hipLaunchKernelGGL(k_gather_u64_by_perm, dim3(grid), dim3(TG_BLOCK), 0, s->stream,
                       d_image, d_perm, n, d_keys);
    TG_HIP_CHECK(hipGetLastError());
    TG_TRY(run_sort_pairs(s, d_keys, d_perm, n));
    if (rank_bits) {
        hipLaunchKernelGGL(k_gather_u64_by_perm, dim3(grid), dim3(TG_BLOCK), 0, s->stream,
                           d_rank, d_perm, n, d_keys);
        TG_HIP_CHECK(hipGetLastError());
        TG_TRY(run_sort_pairs_bits(s, d_keys, d_perm, n, rank_bits));
    }
    TG_HIP_CHECK(hipMemsetAsync(d_state, 0, 8, s->stream));
    hipLaunchKernelGGL(k_var_flags, dim3(grid), dim3(TG_BLOCK), 0, s->stream, d_perm,
                       d_rank, d_image, d_len, n, seen_bytes, d_a, d_state);
    TG_HIP_CHECK(hipGetLastError());
    TG_TRY(run_scan_i32(s, d_a, n + 1, d_state + 1));
    hipLaunchKernelGGL(k_var_scatter_ranks, dim3(grid), dim3(TG_BLOCK), 0, s->stream,
                       d_perm, d_a, n, d_rank);
    TG_HIP_CHECK(hipGetLastError());
    TG_HIP_CHECK(hipMemcpyAsync(h_state, d_state, 8, hipMemcpyDeviceToHost, s->stream));
    TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    return TG_OK;
}

static int bits_for_ranks(int64_t count)
{
    int bits = 1;
    while (bits < 63 && ((int64_t)1 << bits) < count) bits++;
    return bits;
}

/* kf[flat row] = the sortable image of VARCHAR channel `ch`: the row's dense
 * rank among the channel's non-NULL strings in unsigned byte order (a proper
 * prefix first), bit-inverted for DESC, 0 where NULL */
static tg_status varchar_key_image(tg_session* s, const std::vector<DevPage>& pages,
                                   const std::vector<int64_t>& page_base, int32_t ch,
                                   int32_t desc, int64_t n, uint64_t* kf)
{
    PoolScratch ps(s);   /* the refinement's own temporaries go back before the key sorts */
    uint64_t* d_image = nullptr; uint64_t* d_keys = nullptr; int64_t* d_perm = nullptr;
    int32_t* d_len = nullptr; int32_t* d_a = nullptr; int32_t* d_state = nullptr;
    TG_TRY(ps.alloc(&d_image, n * 8));
    TG_TRY(ps.alloc(&d_keys, n * 8));
    TG_TRY(ps.alloc(&d_perm, n * 8));
    TG_TRY(ps.alloc(&d_len, n * 4));
    TG_TRY(ps.alloc(&d_a, (n + 1) * 4));
    TG_TRY(ps.alloc(&d_state, 16));   /* more, new groups, seen NULL, seen '' */
    int32_t* d_seen = d_state + 2;
    TG_HIP_CHECK(hipMemsetAsync(d_state, 0, 16, s->stream));
    TG_HIP_CHECK(hipMemsetAsync(kf, 0, n * 8, s->stream));   /* rank = 0 */
    hipLaunchKernelGGL(k_iota_i64, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0, s->stream,
                       d_perm, n);
    TG_HIP_CHECK(hipGetLastError());
    for (size_t p = 0; p < pages.size(); p++) {
        const DevBlock& b = pages[p].blocks[ch];
        if (!pages[p].n) continue;
        hipLaunchKernelGGL(k_var_lens, dim3(tg_grid_for(pages[p].n)), dim3(TG_BLOCK), 0,
                           s->stream, b.offsets, b.valid, pages[p].n,
                           d_len + page_base[p], d_seen);
        TG_HIP_CHECK(hipGetLastError());
    }
    int32_t h_state[2] = {0, 0};   /* more, rank count - 1 */
    for (int32_t round = 0;; round++) {
        for (size_t p = 0; p < pages.size(); p++) {
            const DevBlock& b = pages[p].blocks[ch];
            if (!pages[p].n) continue;
            hipLaunchKernelGGL(k_var_chunks, dim3(tg_grid_for(pages[p].n)), dim3(TG_BLOCK), 0,
                               s->stream, (const uint8_t*)b.data, b.offsets,
                               d_len + page_base[p], pages[p].n, round,
                               d_image + page_base[p]);
            TG_HIP_CHECK(hipGetLastError());
        }
        int rank_bits = round ? bits_for_ranks((int64_t)h_state[1] + 1) : 0;
        TG_TRY(var_refine_round(s, n, d_image, d_len, 8 * ((int64_t)round + 1), rank_bits,
                                kf, d_perm, d_keys, d_a, d_state, h_state));
        if (!h_state[0]) break;
    }
    /* rows that still tie differ by trailing 0x00 bytes at most: the shorter
     * is a proper prefix of the longer. All ranks distinct: nothing ties. */
    if ((int64_t)h_state[1] + 1 < n) {
        hipLaunchKernelGGL(k_var_len_image, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0,
                           s->stream, d_len, n, d_image);
        TG_HIP_CHECK(hipGetLastError());
        TG_TRY(var_refine_round(s, n, d_image, d_len, INT64_MAX,
                                bits_for_ranks((int64_t)h_state[1] + 1),
                                kf, d_perm, d_keys, d_a, d_state, h_state));
    }
    for (size_t p = 0; p < pages.size(); p++) {
        if (!pages[p].n) continue;
        hipLaunchKernelGGL(k_var_finish, dim3(tg_grid_for(pages[p].n)), dim3(TG_BLOCK), 0,
                           s->stream, pages[p].blocks[ch].valid, desc, pages[p].n,
                           d_seen, kf + page_base[p]);
        TG_HIP_CHECK(hipGetLastError());
    }
    return TG_OK;
}

extern "C" tg_status tg_varchar_chunk_host(const uint8_t* bytes, int32_t len, int32_t round,
                                           uint64_t* out)
{
    if (!out || len < 0 || round < 0 || (!bytes && len > 0)) {
        TG_SET_ERR("tg_varchar_chunk_host: null argument or negative length / round");
        return TG_ERR_INVALID_ARG;
    }
    *out = varchar_chunk(bytes, len, round);
    return TG_OK;
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
        /* a string channel's image is computed over all pages at once */
        bool varchar = !pages.empty() && pages[0].blocks[ch].type == TG_VARCHAR;
        if (varchar && total_rows)
            TG_TRY(varchar_key_image(s, pages, page_base, ch, desc, total_rows, kf[j]));
        for (size_t p = 0; p < pages.size(); p++) {
            const DevBlock& b = pages[p].blocks[ch];
            if (!pages[p].n) continue;
            if (!varchar) {
                hipLaunchKernelGGL(k_topn_keys, dim3(tg_grid_for(pages[p].n)),
                                   dim3(TG_BLOCK), 0, s->stream, b.data, b.valid,
                                   (int32_t)b.type, desc, pages[p].n,
                                   kf[j] + page_base[p]);
                TG_HIP_CHECK(hipGetLastError());
            }
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

/* VARCHAR gather of one source page, lengths pass: output slot o takes the
 * length of flat row idx[o] when it lies in this page; a NULL cell has zero
 * length and clears the output's validity bit */
__global__ void k_pages_var_lens(const int32_t* __restrict__ src_off,
                                 const uint64_t* __restrict__ src_valid,
                                 const int64_t* __restrict__ idx, int64_t take,
                                 int64_t base, int64_t n, int32_t* __restrict__ lens,
                                 uint64_t* __restrict__ out_valid)
{
    int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; o < take; o += stride) {
        int64_t r = idx[o] - base;
        if (r < 0 || r >= n) continue;
        bool isnull = src_valid && !((src_valid[r >> 6] >> (r & 63)) & 1);
        lens[o] = isnull ? 0 : src_off[r + 1] - src_off[r];
        if (isnull)
            atomicAnd((unsigned long long*)&out_valid[o >> 6], ~(1ull << (o & 63)));
    }
}

/* byte copy of one source page: LANES adjacent lanes share a row and copy
 * its bytes b = lane, lane + LANES, ..., so one load of the group touches
 * LANES consecutive bytes. Bytes are copied singly: source and destination
 * start at unrelated alignments. The length comes from the output offsets,
 * so a NULL cell copies nothing. */
template <int LANES>
__global__ void k_pages_var_copy(const uint8_t* __restrict__ src_bytes,
                                 const int32_t* __restrict__ src_off,
                                 const int64_t* __restrict__ idx, int64_t take,
                                 int64_t base, int64_t n,
                                 const int32_t* __restrict__ out_off,
                                 uint8_t* __restrict__ out_bytes)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x / LANES;
    int32_t lane = (int32_t)(t % LANES);
    for (int64_t o = t / LANES; o < take; o += stride) {
        int64_t r = idx[o] - base;
        if (r < 0 || r >= n) continue;
        int32_t len = out_off[o + 1] - out_off[o];
        const uint8_t* sp = src_bytes + src_off[r];
        uint8_t* dp = out_bytes + out_off[o];
        for (int32_t b = lane; b < len; b += LANES) dp[b] = sp[b];
    }
}

/* lanes per row from the mean output length: 4 / 8 / 16 / 32 lanes up to a
 * mean of 16 / 48 / 160 bytes / above. Measured (profiles/order_by_cost.txt):
 * through a sorted, hence scattered, index list 4 lanes beat 1 at 10-byte
 * rows and 8 beat 1 at 40-byte rows, end to end; through an identity list 16
 * lanes are fastest at 100 bytes and 32 at 400. Only through an identity list
 * is a single lane fastest at 3 and 30 bytes, and an ordering operator's
 * index list is not one. */
static int var_copy_lanes(int64_t total_bytes, int64_t take)
{
    /* TG_VAR_COPY_LANES = 1 | 2 | 4 | ... | 64 overrides the table: the knob
     * tools/measure_order_by_cost.py --case sweep turns */
    if (const char* e = getenv("TG_VAR_COPY_LANES")) {
        int v = atoi(e);
        if (v >= 1 && v <= 64 && !(v & (v - 1))) return v;
    }
    int64_t mean = take ? total_bytes / take : 0;
    return mean <= 16 ? 4 : mean <= 48 ? 8 : mean <= 160 ? 16 : 32;
}

/* one VARCHAR channel of gather_pages: lengths per source page, a scan to
 * offsets, one byte-copy launch per source page. b.valid is set up already. */
static tg_status gather_pages_var(tg_session* s, const std::vector<DevPage>& pages,
                                  const std::vector<int64_t>& page_base, size_t c,
                                  const int64_t* d_idx, int64_t take, DevBlock& b)
{
    PoolScratch ps(s);
    int32_t* d_total = nullptr;
    TG_TRY(ps.alloc(&d_total, 4));
    TG_POOL_ALLOC(s, &b.offsets, (take + 1) * 4);
    TG_HIP_CHECK(hipMemsetAsync(b.offsets, 0, (take + 1) * 4, s->stream));
    for (size_t p = 0; take && p < pages.size(); p++) {
        const DevBlock& sb = pages[p].blocks[c];
        if (!pages[p].n) continue;
        hipLaunchKernelGGL(k_pages_var_lens, dim3(tg_grid_for(take)), dim3(TG_BLOCK), 0,
                           s->stream, sb.offsets, sb.valid, d_idx, take, page_base[p],
                           pages[p].n, b.offsets, b.valid);
        TG_HIP_CHECK(hipGetLastError());
    }
    int32_t total = 0;
    if (take) {
        TG_TRY(run_scan_i32(s, b.offsets, take, d_total));
        TG_HIP_CHECK(hipMemcpyAsync(b.offsets + take, d_total, 4, hipMemcpyDeviceToDevice,
                                    s->stream));
        TG_HIP_CHECK(hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, s->stream));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    }
    TG_POOL_ALLOC(s, &b.data, total ? total : 1);
    int lanes = var_copy_lanes(total, take);
    for (size_t p = 0; total && p < pages.size(); p++) {
        const DevBlock& sb = pages[p].blocks[c];
        int64_t pn = pages[p].n;
        if (!pn) continue;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(tg_grid_for(take * lanes)), dim3(TG_BLOCK), 0,
                               s->stream, (const uint8_t*)sb.data, sb.offsets, d_idx, take,
                               page_base[p], pn, b.offsets, (uint8_t*)b.data);
        };
        switch (lanes) {
            case 1: launch(k_pages_var_copy<1>); break;
            case 2: launch(k_pages_var_copy<2>); break;
            case 4: launch(k_pages_var_copy<4>); break;
            case 8: launch(k_pages_var_copy<8>); break;
            case 16: launch(k_pages_var_copy<16>); break;
            case 32: launch(k_pages_var_copy<32>); break;
            default: launch(k_pages_var_copy<64>); break;
        }
        TG_HIP_CHECK(hipGetLastError());
    }
    return TG_OK;
}

/* one gather launch per (channel, source page): each output slot finds its
 * flat row in exactly one page; validity travels along */
tg_status gather_pages(tg_session* s, const std::vector<DevPage>& pages,
                       const std::vector<tg_type>& types, const int64_t* d_idx,
                       int64_t take, DevPage* outp,
                       const std::vector<int32_t>* out_channels)
{
    std::vector<int64_t> page_base = page_bases(pages);
    outp->n = take;
    size_t n_out = out_channels ? out_channels->size() : types.size();
    for (size_t k = 0; k < n_out; k++) {
        size_t c = out_channels ? (size_t)(*out_channels)[k] : k;
        /* in the page before it owns anything: an error frees it with the page */
        outp->blocks.emplace_back();
        DevBlock& b = outp->blocks.back();
        b.type = types[c];
        b.n = take;
        if (channel_nullable(pages, c)) {
            int64_t words = (take + 63) / 64;
            TG_POOL_ALLOC(s, &b.valid, (words ? words : 1) * 8);
            TG_HIP_CHECK(hipMemsetAsync(b.valid, 0xFF, words * 8, s->stream));
        }
        if (b.type == TG_VARCHAR) {
            TG_TRY(gather_pages_var(s, pages, page_base, c, d_idx, take, b));
            continue;
        }
        TG_POOL_ALLOC(s, &b.data, (take ? take : 1) * b.elem_size());
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
