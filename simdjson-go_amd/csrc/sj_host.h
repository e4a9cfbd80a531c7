// sj_host.h -- host-side helpers of the parse driver (no device code).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace sj {

// bytes.TrimSpace as called by parseMessage (parse_json_amd64.go:55): ASCII fast path, and the
// Unicode White_Space set (unicode.IsSpace) once a byte >= 0x80 is met at either end.
namespace trim_detail {
inline bool ascii_ws(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
inline bool uni_ws(uint32_t r) {
    if (r < 0x100) return r == ' ' || (r >= '\t' && r <= '\r') || r == 0x85 || r == 0xa0;
    return r == 0x1680 || (r >= 0x2000 && r <= 0x200a) || r == 0x2028 || r == 0x2029 || r == 0x202f || r == 0x205f ||
           r == 0x3000;
}
// strict UTF-8 decoder (utf8.DecodeRune): malformed => U+FFFD, width 1
inline uint32_t decode(const uint8_t *p, size_t n, size_t *w) {
    *w = 1;
    if (n == 0) return 0xfffd;
    const uint8_t a = p[0];
    if (a < 0x80) return a;
    int need;
    uint32_t r, lo = 0x80, hi = 0xbf;
    if (a >= 0xc2 && a <= 0xdf) { need = 1; r = a & 0x1f; }
    else if (a >= 0xe0 && a <= 0xef) { need = 2; r = a & 0x0f; if (a == 0xe0) lo = 0xa0; if (a == 0xed) hi = 0x9f; }
    else if (a >= 0xf0 && a <= 0xf4) { need = 3; r = a & 0x07; if (a == 0xf0) lo = 0x90; if (a == 0xf4) hi = 0x8f; }
    else return 0xfffd;
    if (n < (size_t)need + 1) return 0xfffd;
    for (int k = 1; k <= need; k++) {
        const uint8_t c = p[k];
        const uint32_t l = k == 1 ? lo : 0x80, h = k == 1 ? hi : 0xbf;
        if (c < l || c > h) return 0xfffd;
        r = (r << 6) | (c & 0x3f);
    }
    *w = (size_t)need + 1;
    return r;
}
inline uint32_t decode_last(const uint8_t *p, size_t n, size_t *w) {  // utf8.DecodeLastRune
    *w = 1;
    if (n == 0) return 0xfffd;
    if (p[n - 1] < 0x80) return p[n - 1];
    const size_t lim = n >= 4 ? n - 4 : 0;
    size_t start = n - 1;
    while (start > lim && (p[start] & 0xc0) == 0x80) start--;
    size_t ww;
    const uint32_t r = decode(p + start, n - start, &ww);
    if (start + ww != n) return 0xfffd;
    *w = ww;
    return r;
}
}  // namespace trim_detail

inline void trim_space(const uint8_t *s, size_t n, size_t *off, size_t *len) {
    using namespace trim_detail;
    size_t a = 0, b = n;
    bool unicode = false;
    for (; a < b; a++) {
        if (s[a] >= 0x80) { unicode = true; break; }
        if (!ascii_ws(s[a])) break;
    }
    if (!unicode)
        for (; b > a; b--) {
            if (s[b - 1] >= 0x80) { unicode = true; break; }
            if (!ascii_ws(s[b - 1])) break;
        }
    if (unicode) {  // TrimFunc(s[a:b], unicode.IsSpace)
        while (a < b) {
            size_t w;
            if (!uni_ws(decode(s + a, b - a, &w))) break;
            a += w;
        }
        while (b > a) {
            size_t w;
            if (!uni_ws(decode_last(s + a, b - a, &w))) break;
            b -= w;
        }
    }
    *off = a;
    *len = b - a;
}

// ---- the windows of a sharded ND message (multi_api.hip multi_parse, sjhip/ndshard.py parse_shard) -------------------------
// The reference trims the message ONCE (pj.Message = bytes.TrimSpace(msg), parse_json_amd64.go:55) and parses every byte
// between two records as it stands: a '\f' behind a record is a stage-2 error there.  So a shard is
//   its cut range  [cut k, cut k+1)   cut k+1 = right behind the first '\n' at or after max(cut k, len * (k+1) / n), the last = len
//   intersected with the global TrimSpace window of the message
//   without the four JSON whitespace bytes at its ends -- and nothing else: '\v', '\f', U+0085, U+00A0, U+2028 ... stay and fail
// A window may be empty (it contributes nothing).
inline bool json_ws(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

// the end of shard k of n: `first_newline(at)` = position of the first '\n' at or behind `at`, len if there is none
template <typename FindNewline>
inline size_t shard_cut_end(size_t len, size_t prev_cut, size_t k, size_t n, FindNewline first_newline) {
    if (k + 1 >= n) return len;
    size_t target = (size_t)((unsigned __int128)len * (k + 1) / n);
    if (target < prev_cut) target = prev_cut;
    const size_t nl = target < len ? first_newline(target) : len;
    return nl < len ? nl + 1 : len;
}

// [a, b) clipped to the global window [g_off, g_off + g_len); an empty result has a == b
inline void shard_clip(size_t *a, size_t *b, size_t g_off, size_t g_len) {
    if (*a < g_off) *a = g_off;
    if (*b > g_off + g_len) *b = g_off + g_len;
    if (*b < *a) *b = *a;
}

// host message: the window of every shard (absolute start, length) and the global window
inline void shard_windows(const uint8_t *msg, size_t len, size_t n, size_t *starts, size_t *lens, size_t *g_off, size_t *g_len) {
    *g_off = *g_len = 0;
    if (len) trim_space(msg, len, g_off, g_len);
    size_t cut = 0;
    for (size_t k = 0; k < n; k++) {
        const size_t end = shard_cut_end(len, cut, k, n, [&](size_t at) {
            const void *nl = memchr(msg + at, '\n', len - at);
            return nl ? (size_t)((const uint8_t *)nl - msg) : len;
        });
        size_t a = cut, b = end;
        shard_clip(&a, &b, *g_off, *g_len);
        while (a < b && json_ws(msg[a])) a++;
        while (b > a && json_ws(msg[b - 1])) b--;
        starts[k] = a;
        lens[k] = b - a;
        cut = end;
    }
}

// A shard in front of the last non-empty one ends where the whole message goes on: "the last structural is a closing bracket"
// (stage1_find_marks_amd64.go:120-129) is asked of the END of the message only.  Such a shard whose window ends otherwise --
// a stray byte or a scalar behind its last record, a record broken across a newline -- is what stage 2 of the whole message
// rejects (stage2_build_tape_amd64.go:196-221), and SJHIP_FLAG_INNER_SHARD makes sjhip_parse_shard_begin say so.
inline void shard_inner(const size_t *lens, size_t n, uint8_t *inner) {
    bool later = false;
    for (size_t k = n; k-- > 0;) {
        inner[k] = later ? 1 : 0;
        if (lens[k]) later = true;
    }
}

}  // namespace sj
