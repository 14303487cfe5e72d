/* ops_topn.hip — TopN operator (§8f row 2).
 *
 * Mirrors operator/TopNOperator.java / TopNProcessor: accumulate input pages,
 * keep the top `limit` rows under the given orderings, emit one page in order.
 * Orderings follow Trino's defaults: ASC = nulls last, DESC = nulls first.
 *
 * Input pages stay device-resident. At finish the top-limit row indices are
 * chosen on one of two paths. From 65536 accumulated rows up, the rows are
 * ordered on the device (order_pages, sort_keys.h: a host partial_sort cost
 * tens of ms at Q3's ~1.1M aggregated groups) and the head of the permutation
 * is used where it lies. Below that, the sort-key channels are brought to the
 * host, a partial_sort selects the indices and they are uploaded. Either way
 * the output page is gathered on the device (gather_pages).
 *
 * OrderByOp, below it, is ORDER BY without LIMIT and TopN with VARCHAR
 * channels (tg_order_by_create, tg_topn_create_ex): always the device path.
 */
#include "dev_hash.h"
#include "sort_keys.h"   /* the page check, order_pages, gather_pages */
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
        TG_TRY(check_fixed_width_page("topn", page, types));
        DevPage in;
        TG_TRY(tg_upload_page(s, page, &in));
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

    /* the row indices on either path, then the output gather */
    tg_status emit_into(PoolScratch& ps, int64_t take, DevPage* outp)
    {
        int64_t* d_idx = nullptr;
        std::vector<int64_t> idx;      /* outlives its upload */
        if (device_sortable()) {
            std::vector<std::pair<int32_t, int32_t>> keys;
            for (size_t j = 0; j < sort_channels.size(); j++)
                keys.emplace_back(sort_channels[j], sort_desc[j]);
            TG_TRY(ps.alloc(&d_idx, total_rows * 8));
            TG_TRY(order_pages(s, ps, pages, total_rows, keys, d_idx, nullptr));
        }
        else {
            TG_TRY(host_order(take, &idx));
            TG_TRY(ps.alloc(&d_idx, take * 8));
            if (take)
                TG_HIP_CHECK(hipMemcpyAsync(d_idx, idx.data(), take * 8,
                                            hipMemcpyHostToDevice, s->stream));
        }
        TG_TRY(gather_pages(s, pages, types, d_idx, take, outp));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        return TG_OK;
    }

    tg_status emit()
    {
        DevPage outp;
        tg_status st;
        {
            PoolScratch ps(s);
            st = emit_into(ps, std::min<int64_t>(limit, total_rows), &outp);
        }
        if (st != TG_OK) {
            tg_free_page(s, &outp);
            return st;
        }
        stage_output(std::move(outp));
        for (auto& p : pages) tg_free_page(s, &p);
        pages.clear();
        return TG_OK;
    }

    /* the top `take` flat row indices in order, by a host partial_sort */
    tg_status host_order(int64_t take, std::vector<int64_t>* out)
    {
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
        std::vector<int64_t>& idx = *out;
        idx.resize(total_rows);
        for (int64_t i = 0; i < total_rows; i++) idx[i] = i;
        std::partial_sort(idx.begin(), idx.begin() + take, idx.end(), less);
        idx.resize(take);
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
    /* fixed-width channels only here; VARCHAR goes through tg_topn_create_ex */
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

/* ---- OrderBy / TopN with VARCHAR (tg_order_by_create, tg_topn_create_ex) ----
 * operator/OrderByOperator.java, and TopNOperator over any channel types.
 * One operator: every accumulated row is ordered on the device (order_pages;
 * a VARCHAR key sorts by its rank image) and the first `take`
 * rows are gathered through output_channels (gather_pages). `limit` is absent
 * (< 0) for OrderBy. No host path and no row threshold: whole-key ties keep
 * input order at every row count. */
struct OrderByOp : tg_operator {
    const char* name = "order_by";
    std::vector<tg_type> types;
    std::vector<int32_t> sort_channels;
    std::vector<int32_t> sort_desc;     /* 0 asc, 1 desc */
    std::vector<int32_t> output_channels;
    int64_t limit = -1;                 /* < 0: every row */
    std::vector<DevPage> pages;
    std::vector<int64_t> var_bytes;     /* per channel: VARCHAR bytes accumulated */
    int64_t total_rows = 0;
    bool emitted = false;

    tg_status add_input(const tg_page* page) override
    {
        TG_TRY(check_page(name, page, types));
        /* output offsets are int32 and the scans count rows in int32: sums on
         * the host */
        if (total_rows + page->position_count > INT32_MAX) {
            TG_SET_ERR("%s: more than INT32_MAX rows accumulated", name);
            return TG_ERR_UNSUPPORTED;
        }
        DevPage in;
        tg_status st = tg_upload_page(s, page, &in);
        /* the bytes a VARCHAR block carries, offsets[n], as the upload read
         * them: no second trip to a device-resident page */
        for (size_t c = 0; st == TG_OK && c < types.size(); c++)
            if (types[c] == TG_VARCHAR && var_bytes[c] + in.blocks[c].var_bytes > INT32_MAX) {
                TG_SET_ERR("%s: VARCHAR channel %zu accumulates more than INT32_MAX bytes",
                           name, c);
                st = TG_ERR_UNSUPPORTED;
            }
        if (st != TG_OK) {
            tg_free_page(s, &in);
            return st;
        }
        for (size_t c = 0; c < types.size(); c++) var_bytes[c] += in.blocks[c].var_bytes;
        total_rows += in.n;
        pages.emplace_back(std::move(in));
        return TG_OK;
    }

    /* the order, then the output gather, then one stream sync */
    tg_status emit_into(PoolScratch& ps, int64_t take, DevPage* outp)
    {
        std::vector<std::pair<int32_t, int32_t>> keys;
        for (size_t j = 0; j < sort_channels.size(); j++)
            keys.emplace_back(sort_channels[j], sort_desc[j]);
        int64_t* d_idx = nullptr;
        TG_TRY(ps.alloc(&d_idx, total_rows * 8));
        TG_TRY(order_pages(s, ps, pages, total_rows, keys, d_idx, nullptr));
        TG_TRY(gather_pages(s, pages, types, d_idx, take, outp, &output_channels));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        return TG_OK;
    }

    tg_status emit()
    {
        if (total_rows) {
            DevPage outp;
            tg_status st;
            {
                PoolScratch ps(s);
                st = emit_into(ps, limit < 0 ? total_rows : std::min(limit, total_rows), &outp);
            }
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

    ~OrderByOp() override
    {
        for (auto& p : pages) tg_free_page(s, &p);
        for (auto& p : out_pages_) tg_free_page(s, &p);
    }
};

/* every check of both entry points; limit < 0 = OrderBy */
static tg_status order_by_create(const char* name, tg_session* s,
    const int32_t* types, int32_t n_channels,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    const int32_t* output_channels, int32_t n_output, int64_t limit, tg_operator** out)
{
    if (!s || !types || !out || n_channels < 1 || n_sort < 1 || n_output < 0 ||
        !sort_channels || !sort_desc || (!output_channels && n_output > 0)) {
        TG_SET_ERR("invalid %s spec", name);
        return TG_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n_channels; i++)
        if (types[i] < TG_BIGINT || types[i] > TG_VARCHAR) {
            TG_SET_ERR("%s: unknown type %d of channel %d", name, types[i], i);
            return TG_ERR_INVALID_ARG;
        }
    for (int i = 0; i < n_sort; i++)
        if (sort_channels[i] < 0 || sort_channels[i] >= n_channels) {
            TG_SET_ERR("%s sort channel %d outside %d channels", name, sort_channels[i], n_channels);
            return TG_ERR_INVALID_ARG;
        }
    for (int i = 0; i < n_output; i++)
        if (output_channels[i] < 0 || output_channels[i] >= n_channels) {
            TG_SET_ERR("%s output channel %d outside %d channels", name, output_channels[i], n_channels);
            return TG_ERR_INVALID_ARG;
        }
    auto* op = new OrderByOp();
    op->s = s;
    op->name = name;
    for (int i = 0; i < n_channels; i++) op->types.push_back((tg_type)types[i]);
    op->sort_channels.assign(sort_channels, sort_channels + n_sort);
    for (int i = 0; i < n_sort; i++) op->sort_desc.push_back(sort_desc[i] ? 1 : 0);
    if (n_output) op->output_channels.assign(output_channels, output_channels + n_output);
    else for (int i = 0; i < n_channels; i++) op->output_channels.push_back(i);
    op->var_bytes.assign(n_channels, 0);
    op->limit = limit;
    *out = op;
    return TG_OK;
}

extern "C" tg_status tg_order_by_create(tg_session* s,
    const int32_t* types, int32_t n_channels,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    const int32_t* output_channels, int32_t n_output, tg_operator** out)
{
    return order_by_create("order_by", s, types, n_channels, sort_channels, sort_desc, n_sort,
                           output_channels, n_output, -1, out);
}

extern "C" tg_status tg_topn_create_ex(tg_session* s,
    const int32_t* types, int32_t n_channels,
    const int32_t* sort_channels, const int32_t* sort_desc, int32_t n_sort,
    int32_t limit, tg_operator** out)
{
    if (limit < 1) {
        TG_SET_ERR("topn_ex: limit %d < 1", limit);
        return TG_ERR_INVALID_ARG;
    }
    return order_by_create("topn_ex", s, types, n_channels, sort_channels, sort_desc, n_sort,
                           nullptr, 0, limit, out);
}
