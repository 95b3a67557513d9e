// The rule of K-DEFLATE (blocked-gzip output, `--gz-out`) in one place, for the host layer, the kernel's bounds (pf_deflate.hip) and the
// stand-alone test (tests/cpp/test_deflate_rule.cpp): the encoder of pf_deflate_core.hpp -- parse, coding, block choice and container are
// defined in words there -- run as lane 0 of 1 over plain memory, and the cut of a text into members.
//
// A file written with `--gz-out` is its text cut into members of 65 280 bytes (bgzip's cut), the last one shorter, then the 28-byte
// end-of-file marker: a function of the text alone.
#pragma once
#include <stdint.h>
#include <string.h>

#include "pf_deflate_core.hpp"

namespace pf_deflate {

// the 28-byte end-of-file marker: what the encoder makes of no text
constexpr uint8_t EOF_MARKER[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

inline uint64_t n_members(uint64_t n_bytes, uint32_t member_text) { return (n_bytes + member_text - 1) / member_text; }
// the bytes that hold any n_bytes of text cut into members of member_text
inline uint64_t bound(uint64_t n_bytes, uint32_t member_text) { return n_bytes + MEMBER_EXTRA * n_members(n_bytes, member_text); }

struct HostText {
    const uint8_t *p;
    uint32_t n;
    uint32_t word(uint32_t i) const {
        uint32_t w = 0;
        for (uint32_t b = 0; b < 4; ++b)
            if (i + b < n) w |= (uint32_t)p[i + b] << (8 * b);
        return w;
    }
};
struct HostOut {   // over zeros
    uint8_t *p;
    void put(uint32_t bitpos, uint64_t value, uint32_t nbits) {
        if (!nbits) return;
        value &= nbits >= 64 ? ~0ull : ((1ull << nbits) - 1ull);
        uint64_t v = value << (bitpos & 7u);   // nbits <= 57
        for (uint32_t at = bitpos >> 3; v; ++at, v >>= 8) p[at] |= (uint8_t)v;
    }
};

// what the caller lends one call of deflate_member
struct HostWork {
    Codes codes;
    uint16_t head[HASH_SIZE];         // position + 1 of the last p inserted with this hash
    uint32_t token[MEMBER_TEXT];      // in order: a literal's byte, or 1 << 31 | (len - 3) << 16 | (dist - 1)
};
struct Result { uint32_t kind, literals, matches; };

// text[0, n), n <= 65280 -> the member at out[0, return value); out holds n + 31 bytes
inline uint32_t deflate_member(const uint8_t *text, uint32_t n, uint8_t *out, HostWork &w, Result *res = nullptr) {
    Codes &c = w.codes;
    const HostText t{text, n};
    memset(w.head, 0, sizeof w.head);
    memset(c.freq_lit, 0, sizeof c.freq_lit);
    memset(c.freq_dist, 0, sizeof c.freq_dist);
    uint32_t n_tok = 0, n_match = 0, next = 0;
    for (uint32_t p = 0; p < n; ++p) {   // every position is inserted; the parse stands on `next`
        uint32_t len = 0, dist = 0;
        if (p + 4 <= n) {
            const uint32_t h = hash4(t.word(p));
            const uint32_t q1 = w.head[h];
            w.head[h] = (uint16_t)(p + 1);
            if (p == next && q1 && p - (q1 - 1) <= MAX_DIST) {
                len = match_len(t, p, q1 - 1, n - p < MAX_MATCH ? n - p : MAX_MATCH);
                dist = p - (q1 - 1);
            }
        }
        if (p != next) continue;
        if (len >= MIN_MATCH) {
            w.token[n_tok++] = (1u << 31) | ((len - 3) << 16) | (dist - 1);
            ++c.freq_lit[len_sym(len).sym];
            ++c.freq_dist[dist_sym(dist).sym];
            ++n_match;
            next = p + len;
        } else {
            w.token[n_tok++] = text[p];
            ++c.freq_lit[text[p]];
            next = p + 1;
        }
    }
    ++c.freq_lit[EOB];
    choose_block(c, n, 0u, 1u, NoSync{});
    const uint32_t size = member_bytes(c);
    memset(out, 0, size);
    HostOut o{out};
    uint32_t at = put_headers(c, n, o);
    if (c.kind == KIND_STORED) {
        if (n) memcpy(out + at / 8, text, n);
    } else {
        if (c.kind == KIND_FIXED) fixed_codes(c, 0u, 1u, NoSync{});
        for (uint32_t i = 0; i < n_tok; ++i) {
            uint64_t v;
            const uint32_t tk = w.token[i];
            const uint32_t nb = (tk >> 31) ? match_bits(c, ((tk >> 16) & 0xffu) + 3, (tk & 0xffffu) + 1, &v) : literal_bits(c, tk, &v);
            o.put(at, v, nb);
            at += nb;
        }
    }
    uint32_t reg = 0xffffffffu;
    for (uint32_t i = 0; i < n; ++i) reg = pf_inflate::crc_byte(reg, text[i]);
    put_end(c, at, ~reg, n, o);
    if (res) *res = Result{c.kind, n_tok - n_match, n_match};
    return size;
}

}  // namespace pf_deflate
