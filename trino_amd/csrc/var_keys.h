/* var_keys.h — the cell function behind the sortable image of a VARCHAR key
 * channel (order_pages, sort.hip). Shared by the device kernel
 * k_var_chunks and the host hook tg_varchar_chunk_host, so the CPU suite
 * checks the very code the kernel runs.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

/* the "chunk" of a string in refinement round `round`: its bytes
 * [8 * round, 8 * round + 8) read big-endian into a u64, positions at or past
 * `len` reading as zero. Unsigned u64 order of the chunks of one round is the
 * unsigned byte order of those eight positions. Never touches a byte at or
 * beyond bytes + len: a string that ends before the round's window is not
 * read at all (bytes may then be null). */
__host__ __device__ static inline uint64_t varchar_chunk(const uint8_t* bytes, int32_t len,
                                                         int32_t round)
{
    int64_t lo = (int64_t)round * 8;
    uint64_t v = 0;
    #pragma unroll
    for (int b = 0; b < 8; b++) {
        int64_t p = lo + b;
        v = (v << 8) | (p < (int64_t)len ? (uint64_t)bytes[p] : 0ull);
    }
    return v;
}
