/* sort_keys.h — sort-key images and permutation gathers shared by the TopN
 * operator (ops_topn.hip) and the Window operator (ops_window.hip).
 *
 * Both order rows by stable radix passes over one u64 image per key channel
 * (run_sort_pairs, least-significant channel first) and gather the payload
 * through the resulting permutation. The kernels are `static`: every operator
 * file that includes this header gets its own copy, so the two translation
 * units do not collide at link time.
 */
#pragma once
#include "common.h"

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

static __global__ void k_topn_keys(const void* __restrict__ data,
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
static __global__ void k_topn_null_keys(const uint64_t* __restrict__ valid, int32_t desc,
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

static __global__ void k_gather_u64_by_perm(const uint64_t* __restrict__ kf,
                                            const int64_t* __restrict__ perm, int64_t n,
                                            uint64_t* __restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = kf[perm[i]];
}

static __global__ void k_iota_topn(int64_t* v, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) v[i] = i;
}
