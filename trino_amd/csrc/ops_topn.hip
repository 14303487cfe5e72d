/* ops_topn.hip — TopN operator (§8f row 2).
 *
 * Mirrors operator/TopNOperator.java / TopNProcessor: accumulate input pages,
 * keep the top `limit` rows under the given orderings, emit one page in order.
 * Orderings follow Trino's defaults: ASC = nulls last, DESC = nulls first.
 *
 * Round-1 shape: input pages stay device-resident; at finish the SORT-KEY
 * channels of the accumulated rows are brought to the host, a partial_sort
 * selects the top-limit indices (limit is small — Q3/most sweep tails use
 * LIMIT 10..100), and the output page is gathered on device. A device top-k
 * selection kernel replaces the host sort when limit*pages grows (tracked in
 * DESIGN.md §8f).
 */
#include "dev_hash.h"
#include "sort_keys.h"   /* topn_sortable, the key kernels and the gathers */
#include <algorithm>

struct TopNOp : tg_operator {
    std::vector<tg_type> types;
    std::vector<int32_t> sort_channels;
    std::vector<int32_t> sort_desc;     /* 0 asc, 1 desc */
    int32_t limit = 0;
    std::vector<DevPage> pages;
    int64_t total_rows = 0;
    bool emitted = false;

    tg_status add_input(const tg_page* page) override
    {
        /* the output gather copies cells at the declared width */
        if (page->channel_count < (int32_t)types.size()) {
            TG_SET_ERR("topn page has %d channels, operator %zu", page->channel_count, types.size());
            return TG_ERR_INVALID_ARG;
        }
        for (size_t c = 0; c < types.size(); c++) {
            DevBlock want, got;
            want.type = types[c];
            got.type = (tg_type)page->blocks[c].type;
            if (got.type == TG_VARCHAR || got.elem_size() != want.elem_size()) {
                TG_SET_ERR("topn channel %zu type %d, operator declared %d", c,
                           page->blocks[c].type, (int)types[c]);
                return TG_ERR_INVALID_ARG;
            }
        }
        DevPage in;
        tg_status st = tg_upload_page(s, page, &in);
        if (st != TG_OK) return st;
        total_rows += in.n;
        pages.emplace_back(std::move(in));
        return TG_OK;
    }

    bool device_sortable() const
    {
        for (int32_t ch : sort_channels)
            if (types[ch] == TG_VARCHAR) return false;
        return total_rows >= 65536;
    }

    /* device top-k: per-channel sortable-u64 keys, then stable radix passes
     * least-significant key first (lexicographic), take the head of the
     * final permutation. Replaces a host partial_sort that cost tens of ms
     * at Q3's ~1.1M aggregated groups. */
    tg_status emit_device(int64_t take, std::vector<int64_t>* idx)
    {
        size_t k = sort_channels.size();
        std::vector<int64_t> page_base(pages.size() + 1, 0);
        for (size_t p = 0; p < pages.size(); p++)
            page_base[p + 1] = page_base[p] + pages[p].n;
        std::vector<uint64_t*> kf(k, nullptr), nf(k, nullptr);
        for (size_t j = 0; j < k; j++) {
            TG_POOL_ALLOC(s, &kf[j], total_rows * 8);
            bool nullable = false;
            for (auto& pg : pages) nullable |= pg.n && pg.blocks[sort_channels[j]].valid;
            if (nullable) TG_POOL_ALLOC(s, &nf[j], total_rows * 8);
            for (size_t p = 0; p < pages.size(); p++) {
                const DevBlock& b = pages[p].blocks[sort_channels[j]];
                if (!pages[p].n) continue;
                hipLaunchKernelGGL(k_topn_keys, dim3(tg_grid_for(pages[p].n)),
                                   dim3(TG_BLOCK), 0, s->stream, b.data, b.valid,
                                   (int32_t)b.type, sort_desc[j], pages[p].n,
                                   kf[j] + page_base[p]);
                TG_HIP_CHECK(hipGetLastError());
                if (!nullable) continue;
                hipLaunchKernelGGL(k_topn_null_keys, dim3(tg_grid_for(pages[p].n)),
                                   dim3(TG_BLOCK), 0, s->stream, b.valid,
                                   sort_desc[j], pages[p].n, nf[j] + page_base[p]);
                TG_HIP_CHECK(hipGetLastError());
            }
        }
        int64_t* d_perm = nullptr;
        uint64_t* d_keys = nullptr;
        TG_POOL_ALLOC(s, &d_perm, total_rows * 8);
        TG_POOL_ALLOC(s, &d_keys, total_rows * 8);
        hipLaunchKernelGGL(k_iota_topn, dim3(tg_grid_for(total_rows)), dim3(TG_BLOCK),
                           0, s->stream, d_perm, total_rows);
        TG_HIP_CHECK(hipGetLastError());
        for (int j = (int)k - 1; j >= 0; j--) {
            hipLaunchKernelGGL(k_gather_u64_by_perm, dim3(tg_grid_for(total_rows)),
                               dim3(TG_BLOCK), 0, s->stream, kf[j], d_perm,
                               total_rows, d_keys);
            TG_HIP_CHECK(hipGetLastError());
            tg_status st = run_sort_pairs(s, d_keys, d_perm, total_rows);
            if (st != TG_OK) return st;
            if (!nf[j]) continue;
            /* the channel's major order: NULL or not, one stable 1-bit pass */
            hipLaunchKernelGGL(k_gather_u64_by_perm, dim3(tg_grid_for(total_rows)),
                               dim3(TG_BLOCK), 0, s->stream, nf[j], d_perm,
                               total_rows, d_keys);
            TG_HIP_CHECK(hipGetLastError());
            st = run_sort_pairs_bits(s, d_keys, d_perm, total_rows, 1);
            if (st != TG_OK) return st;
        }
        idx->resize(take);
        if (take) {
            TG_HIP_CHECK(hipMemcpy(idx->data(), d_perm, take * 8,
                                   hipMemcpyDeviceToHost));
        }
        for (size_t j = 0; j < k; j++) { tg_pool_free(s, kf[j]); tg_pool_free(s, nf[j]); }
        tg_pool_free(s, d_perm);
        tg_pool_free(s, d_keys);
        return TG_OK;
    }

    tg_status emit()
    {
        if (device_sortable()) {
            int64_t take = std::min<int64_t>(limit, total_rows);
            std::vector<int64_t> idx;
            tg_status st = emit_device(take, &idx);
            if (st != TG_OK) return st;
            return gather_out(take, idx);
        }
        /* concatenate sort channels on host */
        size_t k = sort_channels.size();
        std::vector<std::vector<double>> keys_f(k);
        std::vector<std::vector<int64_t>> keys_i(k);
        std::vector<std::vector<uint8_t>> keys_null(k);
        for (size_t j = 0; j < k; j++) {
            int ch = sort_channels[j];
            bool isf = types[ch] == TG_DOUBLE;
            if (isf) keys_f[j].reserve(total_rows); else keys_i[j].reserve(total_rows);
            keys_null[j].reserve(total_rows);
            for (auto& p : pages) {
                const DevBlock& b = p.blocks[ch];
                std::vector<uint64_t> valid;
                if (b.valid) {
                    valid.resize((p.n + 63) / 64);
                    TG_HIP_CHECK(hipMemcpy(valid.data(), b.valid, valid.size() * 8,
                                           hipMemcpyDeviceToHost));
                }
                if (isf) {
                    std::vector<double> tmp(p.n);
                    TG_HIP_CHECK(hipMemcpy(tmp.data(), b.data, p.n * 8, hipMemcpyDeviceToHost));
                    keys_f[j].insert(keys_f[j].end(), tmp.begin(), tmp.end());
                }
                else {
                    std::vector<int64_t> tmp(p.n);
                    switch (b.elem_size()) {
                        case 8: {
                            TG_HIP_CHECK(hipMemcpy(tmp.data(), b.data, p.n * 8, hipMemcpyDeviceToHost));
                            break;
                        }
                        case 4: {
                            std::vector<int32_t> t4(p.n);
                            TG_HIP_CHECK(hipMemcpy(t4.data(), b.data, p.n * 4, hipMemcpyDeviceToHost));
                            for (int64_t i = 0; i < p.n; i++) tmp[i] = t4[i];
                            break;
                        }
                        case 2: {
                            std::vector<int16_t> t2(p.n);
                            TG_HIP_CHECK(hipMemcpy(t2.data(), b.data, p.n * 2, hipMemcpyDeviceToHost));
                            for (int64_t i = 0; i < p.n; i++) tmp[i] = t2[i];
                            break;
                        }
                        default: {
                            std::vector<int8_t> t1(p.n);
                            TG_HIP_CHECK(hipMemcpy(t1.data(), b.data, p.n, hipMemcpyDeviceToHost));
                            for (int64_t i = 0; i < p.n; i++) tmp[i] = t1[i];
                            break;
                        }
                    }
                    keys_i[j].insert(keys_i[j].end(), tmp.begin(), tmp.end());
                }
                for (int64_t i = 0; i < p.n; i++) {
                    bool isnull = b.valid && !((valid[i >> 6] >> (i & 63)) & 1);
                    keys_null[j].push_back(isnull ? 1 : 0);
                }
            }
        }
        /* comparator: channel-ordered; ASC nulls last, DESC nulls first */
        auto less = [&](int64_t a, int64_t b) {
            for (size_t j = 0; j < k; j++) {
                bool desc = sort_desc[j];
                bool na = keys_null[j][a], nb = keys_null[j][b];
                if (na || nb) {
                    if (na != nb) return desc ? na : nb;  /* null first on desc */
                    continue;
                }
                int cmp;
                if (types[sort_channels[j]] == TG_DOUBLE) {
                    /* +-0 tie; every NaN ties with every NaN above +inf: a
                     * strict weak ordering, the same as topn_sortable's */
                    double x = keys_f[j][a], y = keys_f[j][b];
                    bool xn = x != x, yn = y != y;
                    cmp = (xn || yn) ? (int)xn - (int)yn
                                     : (x < y) ? -1 : (x > y) ? 1 : 0;
                }
                else {
                    int64_t x = keys_i[j][a], y = keys_i[j][b];
                    cmp = (x < y) ? -1 : (x > y) ? 1 : 0;
                }
                if (cmp) return desc ? cmp > 0 : cmp < 0;
            }
            return false;
        };
        int64_t take = std::min<int64_t>(limit, total_rows);
        std::vector<int64_t> idx(total_rows);
        for (int64_t i = 0; i < total_rows; i++) idx[i] = i;
        std::partial_sort(idx.begin(), idx.begin() + take, idx.end(), less);
        idx.resize(take);
        return gather_out(take, idx);
    }

    tg_status gather_out(int64_t take, const std::vector<int64_t>& idx)
    {
        /* one gather launch per (channel, source page): each output slot
         * finds its flat row in exactly one page; validity travels along */
        std::vector<int64_t> page_base(pages.size() + 1, 0);
        for (size_t p = 0; p < pages.size(); p++)
            page_base[p + 1] = page_base[p] + pages[p].n;

        int64_t* d_idx = nullptr;
        TG_POOL_ALLOC(s, &d_idx, (take ? take : 1) * 8);
        if (take)
            TG_HIP_CHECK(hipMemcpyAsync(d_idx, idx.data(), take * 8,
                                        hipMemcpyHostToDevice, s->stream));
        DevPage outp;
        outp.n = take;
        for (size_t c = 0; c < types.size(); c++) {
            DevBlock b;
            b.type = types[c];
            b.n = take;
            TG_POOL_ALLOC(s, &b.data, (take ? take : 1) * b.elem_size());
            bool nullable = false;
            for (auto& pg : pages) nullable |= pg.n && pg.blocks[c].valid;
            if (nullable) {
                int64_t words = (take + 63) / 64;
                TG_POOL_ALLOC(s, &b.valid, (words ? words : 1) * 8);
                TG_HIP_CHECK(hipMemsetAsync(b.valid, 0xFF, words * 8, s->stream));
            }
            for (size_t p = 0; take && p < pages.size(); p++) {
                const DevBlock& sb = pages[p].blocks[c];
                int64_t pn = pages[p].n;
                if (!pn) continue;
                dim3 grid(tg_grid_for(take)), block(TG_BLOCK);
                switch (b.elem_size()) {
                    case 8: hipLaunchKernelGGL(k_topn_gather<int64_t>, grid, block, 0, s->stream,
                                (const int64_t*)sb.data, sb.valid, d_idx, take, page_base[p], pn,
                                (int64_t*)b.data, b.valid); break;
                    case 4: hipLaunchKernelGGL(k_topn_gather<int32_t>, grid, block, 0, s->stream,
                                (const int32_t*)sb.data, sb.valid, d_idx, take, page_base[p], pn,
                                (int32_t*)b.data, b.valid); break;
                    case 2: hipLaunchKernelGGL(k_topn_gather<int16_t>, grid, block, 0, s->stream,
                                (const int16_t*)sb.data, sb.valid, d_idx, take, page_base[p], pn,
                                (int16_t*)b.data, b.valid); break;
                    default: hipLaunchKernelGGL(k_topn_gather<int8_t>, grid, block, 0, s->stream,
                                (const int8_t*)sb.data, sb.valid, d_idx, take, page_base[p], pn,
                                (int8_t*)b.data, b.valid); break;
                }
                TG_HIP_CHECK(hipGetLastError());
            }
            outp.blocks.push_back(b);
        }
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        tg_pool_free(s, d_idx);
        stage_output(std::move(outp));
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

    ~TopNOp() override
    {
        for (auto& p : pages) tg_free_page(s, &p);
        for (auto& p : out_pages_) tg_free_page(s, &p);
    }
};

extern "C" tg_status tg_topn_create(tg_session* s,
    const int32_t* types, int32_t n_channels,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    int32_t limit, tg_operator** out)
{
    if (!s || !types || !sort_channels || !sort_desc || limit < 1 || n_sort < 1) {
        TG_SET_ERR("invalid topn spec");
        return TG_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n_sort; i++)
        if (sort_channels[i] < 0 || sort_channels[i] >= n_channels) {
            TG_SET_ERR("topn sort channel %d outside %d channels", sort_channels[i], n_channels);
            return TG_ERR_INVALID_ARG;
        }
    /* the output gather moves fixed-width cells only: no plan needs a VARCHAR
     * channel through TopN yet, so it is rejected rather than mangled */
    for (int i = 0; i < n_channels; i++)
        if (types[i] == TG_VARCHAR) {
            TG_SET_ERR("topn: VARCHAR channel %d is not supported", i);
            return TG_ERR_UNSUPPORTED;
        }
    auto* op = new TopNOp();
    op->s = s;
    for (int i = 0; i < n_channels; i++) op->types.push_back((tg_type)types[i]);
    op->sort_channels.assign(sort_channels, sort_channels + n_sort);
    op->sort_desc.assign(sort_desc, sort_desc + n_sort);
    op->limit = limit;
    *out = op;
    return TG_OK;
}
