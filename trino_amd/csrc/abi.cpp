/* abi.cpp — C-ABI session/error surface of libtrino_gpu (include/trino_gpu.h).
 * Host C++; no CPU compute fallback: session creation fails without a HIP
 * device and every operator entry point requires a session.
 */
#include "common.h"

thread_local std::string tg_error_buf;

extern "C" const char* tg_last_error(void)
{
    return tg_error_buf.c_str();
}

extern "C" const char* tg_version(void)
{
    return "trino_amd 0.1 (gfx950; HIP " __DATE__ ")";
}

extern "C" tg_status tg_session_create(int device_ordinal, tg_session** out)
{
    if (!out) { TG_SET_ERR("null out"); return TG_ERR_INVALID_ARG; }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        TG_SET_ERR("no HIP device available (count=%d, %s) — trino_gpu has no CPU "
                   "fallback by design", count, hipGetErrorName(e));
        return TG_ERR_NO_GPU;
    }
    if (device_ordinal < 0 || device_ordinal >= count) {
        TG_SET_ERR("device %d out of range [0,%d)", device_ordinal, count);
        return TG_ERR_INVALID_ARG;
    }
    TG_HIP_CHECK(hipSetDevice(device_ordinal));
    tg_session* s = new tg_session();
    s->device = device_ordinal;
    {
        size_t freeb = 0, totalb = 0;
        if (hipMemGetInfo(&freeb, &totalb) == hipSuccess && totalb)
            s->mem_cap = (size_t)(totalb * 0.92);
    }
    if (hipStreamCreate(&s->stream) != hipSuccess ||
        hipEventCreate(&s->ev_start) != hipSuccess ||
        hipEventCreate(&s->ev_stop) != hipSuccess) {
        TG_SET_ERR("failed to create stream/events");
        delete s;
        return TG_ERR_HIP;
    }
    *out = s;
    return TG_OK;
}

/* evict the LARGEST cached buffers until `need` more bytes fit under the
 * soft cap. Largest-first keeps the many small latency-sensitive buffers
 * (flag vectors, offsets, states) warm; the previous drop-the-whole-cache
 * fallback fired at the same point of every 22-query sweep cycle and the
 * next query (q15) re-paid tens of ms of fresh hipMallocs every step. */
static void pool_evict_for(tg_session* s, size_t need)
{
    while (!s->pool_free.empty() && s->mem_cap &&
           s->pool_bytes + need > s->mem_cap) {
        auto last = std::prev(s->pool_free.end());
        (void)hipFree(last->second);
        s->pool_bytes -= last->first;
        s->pool_sizes.erase(last->second);
        s->pool_free.erase(last);
    }
}

tg_status tg_pool_alloc(tg_session* s, void** out, size_t bytes)
{
    if (bytes == 0) bytes = 1;
    /* first fit: smallest cached buffer with size in [bytes, 2*bytes] */
    auto it = s->pool_free.lower_bound(bytes);
    if (it != s->pool_free.end() && it->first <= bytes * 2) {
        *out = it->second;
        s->pool_free.erase(it);
        return TG_OK;
    }
    pool_evict_for(s, bytes);
    hipError_t e = hipMalloc(out, bytes);
    while (e == hipErrorOutOfMemory && !s->pool_free.empty()) {
        /* cap estimate was optimistic: evict largest-first and retry */
        (void)hipGetLastError();
        auto last = std::prev(s->pool_free.end());
        (void)hipFree(last->second);
        s->pool_bytes -= last->first;
        s->pool_sizes.erase(last->second);
        s->pool_free.erase(last);
        e = hipMalloc(out, bytes);
    }
    if (e != hipSuccess) {
        /* clear the STICKY per-thread last error: a failed hipMalloc would
         * otherwise surface from the next hipGetLastError() after an
         * unrelated kernel launch (found via the OOM test poisoning the
         * dictionary-filter test that ran after it) */
        (void)hipGetLastError();
        TG_SET_ERR("device OOM allocating %zu bytes", bytes);
        return TG_ERR_OOM;
    }
    s->pool_sizes[*out] = bytes;
    s->pool_bytes += bytes;
    return TG_OK;
}

void tg_pool_free(tg_session* s, void* p)
{
    if (!p) return;
    auto it = s->pool_sizes.find(p);
    if (it == s->pool_sizes.end()) {   /* not pool-owned: direct free */
        (void)hipFree(p);
        return;
    }
    s->pool_free.emplace(it->second, p);
}

extern "C" void tg_session_close(tg_session* s)
{
    if (!s) return;
    if (s->pin_buf) (void)hipHostFree(s->pin_buf);
    tg_q1_scratch_free(s);
    for (auto& kv : s->pool_sizes) (void)hipFree(kv.first);
    (void)hipEventDestroy(s->ev_start);
    (void)hipEventDestroy(s->ev_stop);
    (void)hipStreamDestroy(s->stream);
    delete s;
}

/* device-to-host copy by COMPUTE KERNEL into device-mapped pinned memory
 * (then host memcpy). The SDMA copy engine pays a ~20-50 ms wake-up for
 * the FIRST DtoH after a long kernel-only stretch (q15's 8 MB result
 * download measured 23.9 ms mid-sweep, the repeat 0.4 ms — per-copy
 * trace); the compute path stays warm because the query just used it. */
__global__ void k_copy_out(const uint8_t* __restrict__ src,
                           uint8_t* __restrict__ dst, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t nv = n / 16;
    for (size_t k = i; k < nv; k += stride)
        ((ulonglong2*)dst)[k] = ((const ulonglong2*)src)[k];
    for (size_t k = nv * 16 + i; k < n; k += stride) dst[k] = src[k];
}

extern "C" tg_status tg_copy_dtoh(tg_session* s, void* dst, const void* src, int64_t bytes)
{
    constexpr size_t PIN_MAX = 64ull << 20;
    size_t want = (size_t)bytes < PIN_MAX ? (size_t)bytes : PIN_MAX;
    if (s->pin_cap < want) {
        if (s->pin_buf) (void)hipHostFree(s->pin_buf);
        s->pin_buf = nullptr;
        s->pin_cap = 0;
        size_t cap = 1 << 20;
        while (cap < want) cap <<= 1;
        if (hipHostMalloc(&s->pin_buf, cap, hipHostMallocMapped) == hipSuccess)
            s->pin_cap = cap;
        else (void)hipGetLastError();
    }
    void* pin_dev = nullptr;
    if (s->pin_buf &&
        hipHostGetDevicePointer(&pin_dev, s->pin_buf, 0) != hipSuccess) {
        (void)hipGetLastError();
        pin_dev = nullptr;
    }
    if (!s->pin_buf || !pin_dev) {   /* fallback: plain DtoH */
        TG_HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)bytes,
                                    hipMemcpyDeviceToHost, s->stream));
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        return TG_OK;
    }
    size_t off = 0;
    while (off < (size_t)bytes) {
        size_t chunk = (size_t)bytes - off;
        if (chunk > s->pin_cap) chunk = s->pin_cap;
        int grid = (int)((chunk / 16 + 255) / 256);
        if (grid < 1) grid = 1;
        if (grid > 4096) grid = 4096;
        hipLaunchKernelGGL(k_copy_out, dim3(grid), dim3(256), 0, s->stream,
                           (const uint8_t*)src + off, (uint8_t*)pin_dev, chunk);
        TG_HIP_CHECK(hipGetLastError());
        TG_HIP_CHECK(hipStreamSynchronize(s->stream));
        memcpy((char*)dst + off, s->pin_buf, chunk);
        off += chunk;
    }
    return TG_OK;
}

/* device buffer helpers for host pipeline drivers (tpch_queries) */
extern "C" tg_status tg_device_malloc(tg_session* s, void** out, int64_t bytes)
{
    return tg_pool_alloc(s, out, (size_t)bytes);
}

extern "C" tg_status tg_device_free(tg_session* s, void* p)
{
    tg_pool_free(s, p);
    return TG_OK;
}

extern "C" tg_status tg_copy_dtod(tg_session* s, void* dst_dev, const void* src_dev, int64_t bytes)
{
    TG_HIP_CHECK(hipMemcpyAsync(dst_dev, src_dev, (size_t)bytes,
                                hipMemcpyDeviceToDevice, s->stream));
    TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    return TG_OK;
}

extern "C" tg_status tg_copy_htod(tg_session* s, void* dst_dev, const void* src_host, int64_t bytes)
{
    TG_HIP_CHECK(hipMemcpyAsync(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice, s->stream));
    TG_HIP_CHECK(hipStreamSynchronize(s->stream));
    return TG_OK;
}

/* coarse device-memory accounting (LocalMemoryContext.setBytes analog,
 * lib/trino-memory-context): total bytes ever pooled, and bytes currently
 * cached (free) in the pool. live = total - cached. */
extern "C" tg_status tg_session_memory(tg_session* s, int64_t* total_bytes,
                                       int64_t* cached_bytes)
{
    if (!s) { TG_SET_ERR("null session"); return TG_ERR_INVALID_ARG; }
    int64_t cached = 0;
    for (auto& kv : s->pool_free) cached += (int64_t)kv.first;
    if (total_bytes) *total_bytes = (int64_t)s->pool_bytes;
    if (cached_bytes) *cached_bytes = cached;
    return TG_OK;
}

/* generic stream timer over the session's HIP events: bracket operator
 * calls (all kernels launch on s->stream) for per-phase rooflines in
 * bench.py. start/stop pairs must not nest. */
extern "C" tg_status tg_timer_start(tg_session* s)
{
    TG_HIP_CHECK(hipEventRecord(s->ev_start, s->stream));
    return TG_OK;
}

extern "C" tg_status tg_timer_stop(tg_session* s, double* ms)
{
    TG_HIP_CHECK(hipEventRecord(s->ev_stop, s->stream));
    TG_HIP_CHECK(hipEventSynchronize(s->ev_stop));
    float f = 0.f;
    TG_HIP_CHECK(hipEventElapsedTime(&f, s->ev_start, s->ev_stop));
    *ms = (double)f;
    return TG_OK;
}
