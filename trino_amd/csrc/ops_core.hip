/* ops_core.hip — page upload/decode, expression compile, generic operator
 * C-ABI glue (operator/Operator.java:18-50 surface). */
#include "operators.h"
#include <algorithm>

/* ---- dictionary / RLE decode kernels (collapse to flat values on upload;
 * DictionaryBlock.java:55-58, RunLengthEncodedBlock) ---- */
template <typename T>
__global__ void k_dict_decode(const T* __restrict__ dict, const int32_t* __restrict__ ids,
                              int64_t n, T* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = dict[ids[i]];
}

template <typename T>
__global__ void k_rle_decode(const T* __restrict__ value, int64_t n, T* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    T v = *value;
    for (; i < n; i += stride) out[i] = v;
}

/* validity of a decoded dictionary/RLE block: row i is valid iff the block's
 * own bitmap says so AND the dictionary entry it names is valid (ids ==
 * nullptr: RLE, every row names entry 0). One thread per output word. */
__global__ void k_dict_valid(const uint64_t* __restrict__ outer,
                             const uint64_t* __restrict__ dict_valid,
                             const int32_t* __restrict__ ids, int64_t n,
                             uint64_t* __restrict__ out)
{
    int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t words = (n + 63) / 64;
    for (; w < words; w += stride) {
        uint64_t bits = 0;
        for (int b = 0; b < 64; b++) {
            int64_t i = w * 64 + b;
            if (i >= n) break;
            int64_t id = ids ? ids[i] : 0;
            bits |= ((dict_valid[id >> 6] >> (id & 63)) & 1ull) << b;
        }
        out[w] = outer ? (bits & outer[w]) : bits;
    }
}

tg_status upload_flat(tg_session* s, const void* src, int on_device,
                      int64_t bytes, void** out)
{
    TG_POOL_ALLOC(s, out, bytes);
    TG_HIP_CHECK(hipMemcpyAsync(*out, src, bytes,
                                on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                s->stream));
    return TG_OK;
}

template <typename T>
static tg_status decode_to_flat(tg_session* s, const tg_block* b, DevBlock* out)
{
    int64_t n = b->position_count;
    TG_POOL_ALLOC(s, &out->data, n * sizeof(T));
    if (b->kind == TG_BK_DICTIONARY) {
        const tg_block* d = b->dictionary;
        void* d_dict = nullptr; int32_t* d_ids = nullptr;
        tg_status st = upload_flat(s, d->data, d->on_device, d->position_count * sizeof(T), &d_dict);
        if (st != TG_OK) return st;
        st = upload_flat(s, b->ids, b->on_device, n * sizeof(int32_t), (void**)&d_ids);
        if (st != TG_OK) return st;
        hipLaunchKernelGGL(k_dict_decode<T>, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0, s->stream,
                           (const T*)d_dict, d_ids, n, (T*)out->data);
        TG_HIP_CHECK(hipGetLastError());
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        tg_pool_free(s, d_dict);
        tg_pool_free(s, d_ids);
    }
    else { /* RLE */
        const tg_block* d = b->dictionary;
        void* d_val = nullptr;
        tg_status st = upload_flat(s, d->data, d->on_device, sizeof(T), &d_val);
        if (st != TG_OK) return st;
        hipLaunchKernelGGL(k_rle_decode<T>, dim3(tg_grid_for(n)), dim3(TG_BLOCK), 0, s->stream,
                           (const T*)d_val, n, (T*)out->data);
        TG_HIP_CHECK(hipGetLastError());
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        tg_pool_free(s, d_val);
    }
    return TG_OK;
}

tg_status tg_upload_page(tg_session* s, const tg_page* in, DevPage* out)
{
    out->n = in->position_count;
    out->blocks.resize(in->channel_count);
    for (int c = 0; c < in->channel_count; c++) {
        const tg_block* b = &in->blocks[c];
        DevBlock* db = &out->blocks[c];
        db->type = (tg_type)b->type;
        db->n = b->position_count;
        if (b->type == TG_VARCHAR) {
            if (b->kind != TG_BK_VALUE || !b->offsets) {
                TG_SET_ERR("VARCHAR blocks cross as flat offsets+bytes or "
                           "dictionary-encoded ids");
                return TG_ERR_UNSUPPORTED;
            }
            /* VariableWidthBlock: int32 offsets[n+1] + utf8 bytes */
            int32_t total_bytes = 0;
            if (b->on_device) {
                TG_HIP_CHECK(hipMemcpy(&total_bytes, b->offsets + db->n, 4,
                                       hipMemcpyDeviceToHost));
            }
            else {
                total_bytes = b->offsets[db->n];
            }
            db->var_bytes = total_bytes;
            tg_status st = upload_flat(s, b->offsets, b->on_device,
                                       (db->n + 1) * 4, (void**)&db->offsets);
            if (st != TG_OK) return st;
            st = upload_flat(s, b->data, b->on_device,
                             total_bytes ? total_bytes : 1, &db->data);
            if (st != TG_OK) return st;
            if (b->valid) {
                int64_t words = (db->n + 63) / 64;
                st = upload_flat(s, b->valid, b->on_device, words * 8,
                                 (void**)&db->valid);
                if (st != TG_OK) return st;
            }
            continue;
        }
        if (b->kind == TG_BK_VALUE) {
            if (b->on_device) {
                /* zero-copy borrow: device-resident value blocks flow between
                 * operators without a DtoD pass (the producer keeps them
                 * alive until its close — Operator output contract). */
                db->data = const_cast<void*>(b->data);
                db->owned = false;
            }
            else {
                tg_status st = upload_flat(s, b->data, b->on_device,
                                           db->n * db->elem_size(), &db->data);
                if (st != TG_OK) return st;
            }
        }
        else {
            tg_status st = tg_dispatch_width(db->elem_size(), [&](auto t) {
                return decode_to_flat<decltype(t)>(s, b, db);
            });
            if (st != TG_OK) return st;
            if (b->dictionary && b->dictionary->valid) {
                /* NULL dictionary entries: fold them into the row bitmap */
                const tg_block* d = b->dictionary;
                int64_t words = (db->n + 63) / 64;
                int64_t nd = b->kind == TG_BK_DICTIONARY ? d->position_count : 1;
                uint64_t* d_dv = nullptr; uint64_t* d_outer = nullptr; int32_t* d_ids = nullptr;
                st = upload_flat(s, d->valid, d->on_device, ((nd + 63) / 64) * 8, (void**)&d_dv);
                if (st != TG_OK) return st;
                if (b->kind == TG_BK_DICTIONARY) {
                    st = upload_flat(s, b->ids, b->on_device, db->n * 4, (void**)&d_ids);
                    if (st != TG_OK) return st;
                }
                if (b->valid) {
                    st = upload_flat(s, b->valid, b->on_device, words * 8, (void**)&d_outer);
                    if (st != TG_OK) return st;
                }
                TG_POOL_ALLOC(s, &db->valid, (words ? words : 1) * 8);
                hipLaunchKernelGGL(k_dict_valid, dim3(tg_grid_for(words)), dim3(TG_BLOCK), 0,
                                   s->stream, d_outer, d_dv, d_ids, db->n, db->valid);
                TG_HIP_CHECK(hipGetLastError());
                TG_HIP_CHECK(hipStreamSynchronize(s->stream));
                tg_pool_free(s, d_dv);
                if (d_ids) tg_pool_free(s, d_ids);
                if (d_outer) tg_pool_free(s, d_outer);
                continue;
            }
        }
        if (b->valid) {
            if (b->on_device) {
                db->valid = const_cast<uint64_t*>(b->valid);
                /* owned already false for borrowed VALUE data; for decoded
                 * dictionary/RLE blocks the bitmap is borrowed separately */
                if (db->owned) db->valid_owned_override = true;
            }
            else {
                int64_t words = (db->n + 63) / 64;
                tg_status st = upload_flat(s, b->valid, b->on_device, words * 8,
                                           (void**)&db->valid);
                if (st != TG_OK) return st;
            }
        }
    }
    TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    return TG_OK;
}

void tg_free_page(tg_session* s, DevPage* p)
{
    (void)s;
    for (auto& b : p->blocks) {
        if (b.owned && b.data) tg_pool_free(s, b.data);
        if (b.owned && !b.valid_owned_override && b.valid) tg_pool_free(s, b.valid);
        if (b.owned && b.offsets) tg_pool_free(s, b.offsets);
    }
    p->blocks.clear();
    p->n = 0;
}

/* Copies a validated program (check_expr_depth), rewriting every IN list to
 * its sorted, distinct items: the interpreter searches them where they sit in
 * the program, so host and device copy are the same. A list that directly
 * follows a TG_EXPR_COL can become a term of k_filter_terms; for those the
 * bitmap or the sorted array of its form is uploaded here and owned by `out`. */
tg_status tg_compile_expr(tg_session* s, const tg_expr* e, ExprProgram* out)
{
    out->insts.clear();
    out->sets.clear();
    out->insts.reserve(e->count);
    int n_ops = 0;
    for (int i = 0; i < e->count; i++) {
        const tg_expr_inst& in = e->insts[i];
        n_ops++;
        if (in.op != TG_EXPR_IN_LIST) { out->insts.push_back(in); continue; }
        std::vector<int64_t> items(in.arg0);
        for (int j = 0; j < in.arg0; j++) items[j] = e->insts[i + 1 + j].imm.i64;
        std::sort(items.begin(), items.end());
        items.erase(std::unique(items.begin(), items.end()), items.end());
        InSet set;
        set.pos = (int)out->insts.size();
        set.n = (int)items.size();
        set.mn = items.front();
        set.mx = items.back();
        set.form = in_form_for(set.mn, set.mx);
        tg_expr_inst head = in;
        head.arg0 = set.n;
        out->insts.push_back(head);
        for (int64_t v : items) {
            tg_expr_inst it{};
            it.op = TG_EXPR_IN_ITEM;
            it.imm.i64 = v;
            out->insts.push_back(it);
        }
        bool term = i > 0 && e->insts[i - 1].op == TG_EXPR_COL;
        if (set.form == IN_FORM_MASK) {
            for (int64_t v : items) set.mask |= 1ull << ((uint64_t)v - (uint64_t)set.mn);
        }
        else if (term && set.form == IN_FORM_BITMAP) {
            std::vector<uint64_t> bm(((uint64_t)set.mx - (uint64_t)set.mn) / 64 + 1, 0);
            for (int64_t v : items) {
                uint64_t b = (uint64_t)v - (uint64_t)set.mn;
                bm[b >> 6] |= 1ull << (b & 63);
            }
            tg_status st = upload_flat(s, bm.data(), 0, (int64_t)bm.size() * 8, (void**)&set.d_bitmap);
            if (st == TG_OK && hipStreamSynchronize(s->stream) != hipSuccess) st = TG_ERR_HIP;
            if (st != TG_OK) { out->sets.push_back(set); tg_free_expr(s, out); return st; }
        }
        else if (term) {
            tg_status st = upload_flat(s, items.data(), 0, (int64_t)items.size() * 8, (void**)&set.d_sorted);
            /* the source is a local: the copy ends before it goes away */
            if (st == TG_OK && hipStreamSynchronize(s->stream) != hipSuccess) st = TG_ERR_HIP;
            if (st != TG_OK) { out->sets.push_back(set); tg_free_expr(s, out); return st; }
        }
        out->sets.push_back(set);
        i += in.arg0;
    }
    out->count = (int)out->insts.size();
    /* an item is data, not an operation: the length limit counts the rest */
    if (n_ops > 128) {
        TG_SET_ERR("expression too long (>128 insts)");
        tg_free_expr(s, out);
        return TG_ERR_UNSUPPORTED;
    }
    TG_POOL_ALLOC(s, &out->d_insts, out->count * sizeof(tg_expr_inst));
    TG_HIP_CHECK(hipMemcpyAsync(out->d_insts, out->insts.data(),
                                out->count * sizeof(tg_expr_inst),
                                hipMemcpyHostToDevice, s->stream));
    TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    return TG_OK;
}

extern "C" int32_t tg_expr_in_form(const int64_t* items, int32_t n)
{
    if (!items || n < 1) return -1;
    return (int32_t)in_form_for(*std::min_element(items, items + n),
                                *std::max_element(items, items + n));
}

void tg_free_expr(tg_session* s, ExprProgram* p)
{
    if (p->d_insts) tg_pool_free(s, p->d_insts);
    p->d_insts = nullptr;
    for (auto& set : p->sets) {
        if (set.d_bitmap) tg_pool_free(s, set.d_bitmap);
        if (set.d_sorted) tg_pool_free(s, set.d_sorted);
        set.d_bitmap = nullptr;
        set.d_sorted = nullptr;
    }
}

/* ---- generic operator C ABI ---- */
extern "C" int tg_operator_needs_input(tg_operator* op)
{
    return op ? op->needs_input() : 0;
}

extern "C" tg_status tg_operator_add_input(tg_operator* op, const tg_page* page)
{
    if (!op || !page) { TG_SET_ERR("null arg"); return TG_ERR_INVALID_ARG; }
    if (op->input_finished) { TG_SET_ERR("addInput after finish"); return TG_ERR_STATE; }
    return op->add_input(page);
}

extern "C" tg_status tg_operator_get_output(tg_operator* op, tg_page* out, int* finished)
{
    if (!op || !out || !finished) { TG_SET_ERR("null arg"); return TG_ERR_INVALID_ARG; }
    return op->get_output(out, finished);
}

extern "C" tg_status tg_operator_finish(tg_operator* op)
{
    if (!op) { TG_SET_ERR("null arg"); return TG_ERR_INVALID_ARG; }
    return op->finish();
}

extern "C" void tg_operator_close(tg_operator* op)
{
    delete op;
}
