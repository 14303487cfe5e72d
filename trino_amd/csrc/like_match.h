/* like_match.h — the LIKE matcher shared by the device kernels of
 * tpchgen.hip (k_var_like, k_pool_like, k_pool_like_sorted) and the host
 * hook tg_like_match_host, so the whole matcher can be checked against a
 * reference without a GPU.
 *
 * Pattern language: '%' is the only wildcard ('_' is rejected); everything
 * else is a literal BYTE (no character decoding, no escape). A pattern is up
 * to LIKE_MAX_SEGS literal segments separated by '%':
 *   'abc'     exact:    text == "abc"
 *   'abc%'    prefix    '%abc'  suffix    '%abc%'  floating
 *   'a%b%c'   first segment pinned to the start, last to the end, the ones
 *             between found greedily leftmost, never overlapping
 *   ''        matches only the empty text;  '%', '%%' match every text
 * Mirrors io.trino.type.LikeFunctions / LikePattern matching semantics for
 * patterns without '_' wildcards. */
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LIKE_HD __host__ __device__
#else
#define LIKE_HD
#endif

#define LIKE_MAX_SEGS 4
#define LIKE_MAX_PAT 64
struct LikePat {
    char bytes[LIKE_MAX_PAT];
    int seg_off[LIKE_MAX_SEGS], seg_len[LIKE_MAX_SEGS];
    /* anchor_start/end: the pattern does not begin/end with '%'. The empty
     * pattern has both set and n_segs == 0, which tells it from '%' */
    int n_segs, anchor_start, anchor_end;
};

enum { LIKE_PARSE_OK = 0, LIKE_PARSE_TOO_LONG, LIKE_PARSE_UNDERSCORE,
       LIKE_PARSE_TOO_MANY_SEGS };

LIKE_HD static inline int like_ffsll(unsigned long long m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll(m);
#else
    return __builtin_ffsll((long long)m);
#endif
}

/* SWAR first-byte scan: next index >= from with s[i] == c, else -1
 * (byte-loop scanning measured 38.8 ms for Q13's 150M x ~49 B comments) */
LIKE_HD static inline int like_find_byte(const uint8_t* s, int from,
                                         int len, uint8_t c)
{
    int i = from;
    for (; i < len && ((uintptr_t)(s + i) & 7); i++)
        if (s[i] == c) return i;
    const uint64_t pat = 0x0101010101010101ull * c;
    for (; i + 8 <= len; i += 8) {
        uint64_t w = *(const uint64_t*)(s + i) ^ pat;
        uint64_t m = (w - 0x0101010101010101ull) & ~w & 0x8080808080808080ull;
        if (m) return i + (like_ffsll((unsigned long long)m) - 1) / 8;
    }
    for (; i < len; i++)
        if (s[i] == c) return i;
    return -1;
}

LIKE_HD static inline bool like_match(const uint8_t* txt, int len, const LikePat& p)
{
    /* no '%' at all ('abc' or ''): both anchors pin the one segment, so the
     * text must have exactly its length; the prefix compare below then is
     * the equality test */
    if (p.anchor_start && p.anchor_end && p.n_segs <= 1 &&
        len != (p.n_segs ? p.seg_len[0] : 0)) return false;
    int pos = 0;
    for (int k = 0; k < p.n_segs; k++) {
        int sl = p.seg_len[k];
        const char* seg = p.bytes + p.seg_off[k];
        if (k == 0 && p.anchor_start) {
            if (len < sl) return false;
            for (int i = 0; i < sl; i++) if (txt[i] != (uint8_t)seg[i]) return false;
            pos = sl;
            continue;
        }
        if (k == p.n_segs - 1 && p.anchor_end) {
            if (len - pos < sl) return false;
            for (int i = 0; i < sl; i++)
                if (txt[len - sl + i] != (uint8_t)seg[i]) return false;
            pos = len;
            continue;
        }
        bool found = false;
        int i = pos;
        while (i + sl <= len) {
            i = like_find_byte(txt, i, len - sl + 1, (uint8_t)seg[0]);
            if (i < 0) break;
            bool eq = true;
            for (int j = 1; j < sl && eq; j++) eq = txt[i + j] == (uint8_t)seg[j];
            if (eq) { pos = i + sl; found = true; break; }
            i++;
        }
        if (!found) return false;
    }
    return true;
}

/* host only: split the pattern; LIKE_PARSE_* (the caller words the error) */
static inline int parse_like(const char* pattern, LikePat* p)
{
    memset(p, 0, sizeof(*p));
    size_t L = strlen(pattern);
    if (L >= LIKE_MAX_PAT) return LIKE_PARSE_TOO_LONG;
    p->anchor_start = L == 0 || pattern[0] != '%';
    p->anchor_end = L == 0 || pattern[L - 1] != '%';
    int n = 0, bo = 0;
    const char* q = pattern;
    while (*q) {
        while (*q == '%') q++;
        if (!*q) break;
        const char* e = q;
        while (*e && *e != '%') {
            if (*e == '_') return LIKE_PARSE_UNDERSCORE;
            e++;
        }
        if (n >= LIKE_MAX_SEGS) return LIKE_PARSE_TOO_MANY_SEGS;
        p->seg_off[n] = bo; p->seg_len[n] = (int)(e - q);
        memcpy(p->bytes + bo, q, e - q);
        bo += (int)(e - q);
        n++;
        q = e;
    }
    p->n_segs = n;
    return LIKE_PARSE_OK;
}
