// The part of K-DEFLATE that the kernel (pf_deflate.hip) and the host rule (pf_deflate_rule.hpp) share: an RFC 1951 encoder for one BGZF
// member.  Nothing here allocates, and nothing here touches memory but through the policies
//   Text   word(i): the four bytes at i, least significant first, bytes at and behind n read as zero;
//   Out    put(bitpos, value, nbits): the low nbits (<= 57) of value to the member's bits from bitpos on, over zeros (the bits are OR-ed
//          in, so puts to different bits may come in any order);
//   work   the tables of one member (LDS on the device, the caller's memory on the host).
// lane / n_lanes: the caller's place among those that execute the same call together (host: 0 of 1; kernel: the block's 256 threads,
// all with the same arguments).  What is serial is done by lane 0 between two syncs; the rest is shared.
//
// A member is a pure function of its text t[0, n), n <= 65280:
//   parse    h(p) = (word(p) * 2654435761 mod 2^32) >> 19 for p + 4 <= n (13 bits of the next four bytes).  The candidate of p is the
//            nearest q < p with h(q) = h(p), if p - q <= 32768; every p with p + 4 <= n is inserted, whatever the parse takes.  len(p) =
//            the bytes t[q + i] = t[p + i] from i = 0 on, up to min(258, n - p): q + i may run past p, so a run of one byte is a match of
//            distance 1 and `ACGT` repeated one of distance 4.  The parse is greedy from the left: at p a match with len(p) >= 4 is
//            taken whole (a token of that length and distance p - q) and the parse goes on at p + len(p); anything else is the literal
//            t[p] and the parse goes on at p + 1.
//   coding   frequencies of the tokens' symbols and of the end-of-block code; code lengths by Huffman's construction over the used
//            symbols sorted by (frequency, symbol), limited to 15 bits (7 for the code-length code) by moving the deepest leaves up until
//            Kraft's sum is one, the longest lengths going to the rarest symbols; canonical codes; the dynamic header with its lengths
//            run-length coded (16, 17, 18) over literal/length and distance lengths as one sequence.  A set of one used symbol is one
//            code of one bit; no used distance is HDIST = 0 with one length of zero.
//   block    one block per member: its size as stored (5 + n bytes), fixed and dynamic, in whole bytes; the smallest is written, on
//            equal sizes stored before fixed before dynamic.
//   member   1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | 42 43 02 00 BSIZE - 1 | the block | CRC-32 | ISIZE: at most n + 31 bytes.
// Every loop ends whatever the bytes say: all run over positions, symbols or tree nodes, whose numbers are bounded above.
#pragma once
#include <stdint.h>

#include "pf_inflate_core.hpp"

#if defined(__HIPCC__)
#define PF_DEF_HD __host__ __device__
#else
#define PF_DEF_HD
#endif

namespace pf_deflate {

constexpr uint32_t MEMBER_TEXT = 65280;       // bgzip's cut, 0xff00
constexpr uint32_t HEADER = 18, TRAILER = 8;
constexpr uint32_t MEMBER_EXTRA = 31;         // a member is at most its text and this: header, stored block header, trailer
constexpr int HASH_BITS = 13;
constexpr uint32_t HASH_SIZE = 1u << HASH_BITS;
constexpr uint32_t MIN_MATCH = 4, MAX_MATCH = 258, MAX_DIST = 32768;
constexpr uint32_t N_LIT = 286, N_DIST = 30, N_BL = 19, EOB = 256;
constexpr uint32_t MAX_RLE = N_LIT + N_DIST;
constexpr int LIT_BITS = 15, BL_BITS = 7;
enum Kind { KIND_STORED = 0, KIND_FIXED = 1, KIND_DYNAMIC = 2 };

using pf_inflate::NoSync;

PF_DEF_HD inline uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - HASH_BITS); }

// len(p) against the candidate q < p; max_len = min(258, n - p) >= 1
template <typename Text>
PF_DEF_HD inline uint32_t match_len(const Text &t, uint32_t p, uint32_t q, uint32_t max_len) {
    uint32_t l = 0;
    while (l < max_len) {   // (four bytes a turn)
        const uint32_t x = t.word(p + l) ^ t.word(q + l);
        if (x) { l += (uint32_t)__builtin_ctz(x) >> 3; break; }
        l += 4;
    }
    return l < max_len ? l : max_len;
}

// ---- symbols of a match ----
struct Sym { uint32_t sym, extra, ebits; };
PF_DEF_HD inline Sym len_sym(uint32_t len) {   // 3 .. 258 -> 257 .. 285
    if (len == 258) return Sym{285, 0, 0};
    const uint32_t l = len - 3;
    if (l < 8) return Sym{257 + l, 0, 0};
    const uint32_t k = 31u - (uint32_t)__builtin_clz(l);
    return Sym{257 + 4 * (k - 1) + ((l >> (k - 2)) & 3u), l & ((1u << (k - 2)) - 1u), k - 2};
}
PF_DEF_HD inline Sym dist_sym(uint32_t dist) {   // 1 .. 32768 -> 0 .. 29
    const uint32_t d = dist - 1;
    if (d < 4) return Sym{d, 0, 0};
    const uint32_t k = 31u - (uint32_t)__builtin_clz(d);
    return Sym{2 * k + ((d >> (k - 1)) & 1u), d & ((1u << (k - 1)) - 1u), k - 1};
}
PF_DEF_HD inline uint32_t len_ebits(uint32_t s) { return (s < 265 || s == 285) ? 0u : (s - 261) >> 2; }   // s >= 257
PF_DEF_HD inline uint32_t dist_ebits(uint32_t s) { return s < 4 ? 0u : (s - 2) >> 1; }
PF_DEF_HD inline uint32_t fixed_len(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }

// ---- the tables of one member ----
struct Codes {
    uint32_t freq_lit[N_LIT + 2], freq_dist[N_DIST + 2], freq_bl[N_BL + 1];
    uint8_t len_lit[N_LIT + 2], len_dist[N_DIST + 2], len_bl[N_BL + 1];
    uint16_t code_lit[N_LIT + 2], code_dist[N_DIST + 2], code_bl[N_BL + 1];   // bit-reversed: the first bit of the code is bit 0
    uint16_t rle[MAX_RLE];      // the header's code-length symbols: symbol | extra << 5
    uint32_t n_rle, hlit, hdist, hclen;
    uint32_t kind;              // the block written
    uint32_t bits[3];           // the block's bits as stored, fixed, dynamic
    // the construction's scratch
    uint16_t order[N_LIT + 2];
    uint16_t parent[2 * (N_LIT + 2)];
    uint32_t weight[2 * (N_LIT + 2)];   // a node's frequency, later its depth
    uint32_t used;
};

PF_DEF_HD inline uint32_t bit_reverse(uint32_t code, uint32_t len) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; ++i) { r = (r << 1) | (code & 1u); code >>= 1; }
    return r;
}

// freq[0, n) -> lens[0, n) of at most max_bits, and their canonical codes (bit-reversed).  two: a set of one used symbol is given a second.
template <typename Sync>
PF_DEF_HD inline void build_code(Codes &c, uint32_t *freq, uint32_t n, uint32_t max_bits, bool two, uint8_t *lens, uint16_t *codes, uint32_t lane,
                                 uint32_t n_lanes, const Sync &sync) {
    sync();
    if (lane == 0) {
        uint32_t used = 0;
        for (uint32_t s = 0; s < n; ++s) used += freq[s] ? 1u : 0u;
        if (two && used == 1) { freq[freq[0] ? 1 : 0] = 1; ++used; }   // (counted in the sizes like any other)
        c.used = used;
    }
    sync();
    // shared: every used symbol's place among them by (frequency, symbol)
    for (uint32_t s = lane; s < n; s += n_lanes) {
        lens[s] = 0;
        const uint32_t f = freq[s];
        if (!f) continue;
        uint32_t rank = 0;
        for (uint32_t t = 0; t < n; ++t) {
            const uint32_t g = freq[t];
            rank += (g && (g < f || (g == f && t < s))) ? 1u : 0u;
        }
        c.order[rank] = (uint16_t)s;
    }
    sync();
    if (lane == 0) {
        const uint32_t used = c.used;
        if (used == 1) lens[c.order[0]] = 1;
        if (used >= 2) {
            // Huffman's construction over two queues: the leaves in order, the nodes made so far (their weights ascend too)
            for (uint32_t i = 0; i < used; ++i) c.weight[i] = freq[c.order[i]];
            uint32_t leaf = 0, node = used, made = used;
            while (made < 2 * used - 1) {   // used - 1 turns
                uint32_t pick[2];
                for (int k = 0; k < 2; ++k) {
                    if (leaf < used && (node >= made || c.weight[leaf] <= c.weight[node])) pick[k] = leaf++;
                    else pick[k] = node++;
                }
                c.weight[made] = c.weight[pick[0]] + c.weight[pick[1]];
                c.parent[pick[0]] = (uint16_t)made;
                c.parent[pick[1]] = (uint16_t)made;
                ++made;
            }
            uint32_t count[16];
            for (uint32_t l = 0; l < 16; ++l) count[l] = 0;
            c.weight[made - 1] = 0;   // the root's depth
            for (uint32_t i = made - 1; i-- > 0;) {
                const uint32_t d = c.weight[c.parent[i]] + 1;
                c.weight[i] = d;
                if (i < used) ++count[d < max_bits ? d : max_bits];
            }
            // the limit: leaves deeper than max_bits were counted at max_bits; move leaves up until Kraft's sum is 2^max_bits again
            uint32_t total = 0;
            for (uint32_t l = max_bits; l >= 1; --l) total += count[l] << (max_bits - l);
            while (total > (1u << max_bits)) {   // (a turn takes one off)
                --count[max_bits];
                for (uint32_t l = max_bits - 1; l >= 1; --l)
                    if (count[l]) { --count[l]; count[l + 1] += 2; break; }
                --total;
            }
            uint32_t at = 0;
            for (uint32_t l = max_bits; l >= 1; --l)
                for (uint32_t k = 0; k < count[l]; ++k) lens[c.order[at++]] = (uint8_t)l;
        }
    }
    sync();
    // canonical codes: the counts by every lane alike, a symbol's place among those of its length shared
    uint32_t next[17];
    {
        uint32_t count[17];
        for (uint32_t l = 0; l < 17; ++l) count[l] = 0;
        for (uint32_t s = 0; s < n; ++s) ++count[lens[s]];
        count[0] = 0;
        uint32_t code = 0;
        next[0] = 0;
        for (uint32_t l = 1; l < 17; ++l) { code = (code + count[l - 1]) << 1; next[l] = code; }
    }
    for (uint32_t s = lane; s < n; s += n_lanes) {
        const uint32_t l = lens[s];
        uint32_t rank = 0;
        for (uint32_t t = 0; t < s; ++t) rank += lens[t] == l ? 1u : 0u;
        codes[s] = (uint16_t)(l ? bit_reverse(next[l] + rank, l) : 0u);
    }
    sync();
}

// the dynamic header's symbols from the lengths (lane 0's work): c.rle, c.n_rle, c.hlit, c.hdist, c.freq_bl
PF_DEF_HD inline void rle_lengths(Codes &c) {
    uint32_t hlit = N_LIT, hdist = N_DIST;
    while (hlit > 257 && c.len_lit[hlit - 1] == 0) --hlit;
    while (hdist > 1 && c.len_dist[hdist - 1] == 0) --hdist;
    c.hlit = hlit;
    c.hdist = hdist;
    for (uint32_t s = 0; s < N_BL; ++s) c.freq_bl[s] = 0;
    const uint32_t total = hlit + hdist;
    uint32_t n = 0;
    for (uint32_t i = 0; i < total;) {   // (a turn moves on by at least one length)
        const uint32_t v = i < hlit ? c.len_lit[i] : c.len_dist[i - hlit];
        uint32_t run = 1;
        while (i + run < total && (i + run < hlit ? c.len_lit[i + run] : c.len_dist[i + run - hlit]) == v) ++run;
        uint32_t left = run;
        if (v == 0) {
            while (left >= 11) { const uint32_t r = left < 138 ? left : 138; c.rle[n++] = (uint16_t)(18u | ((r - 11) << 5)); ++c.freq_bl[18]; left -= r; }
            if (left >= 3) { c.rle[n++] = (uint16_t)(17u | ((left - 3) << 5)); ++c.freq_bl[17]; left = 0; }
        } else {
            c.rle[n++] = (uint16_t)v; ++c.freq_bl[v]; --left;
            while (left >= 3) { const uint32_t r = left < 6 ? left : 6; c.rle[n++] = (uint16_t)(16u | ((r - 3) << 5)); ++c.freq_bl[16]; left -= r; }
        }
        while (left) { c.rle[n++] = (uint16_t)v; ++c.freq_bl[v]; --left; }
        i += run;
    }
    c.n_rle = n;
}

PF_DEF_HD inline uint32_t bl_order(uint32_t i) {
    const uint8_t order[N_BL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// From the frequencies of the member's tokens (the end-of-block code counted) to its codes, the three sizes and the kind written.
template <typename Sync>
PF_DEF_HD inline void choose_block(Codes &c, uint32_t n_text, uint32_t lane, uint32_t n_lanes, const Sync &sync) {
    build_code(c, c.freq_lit, N_LIT, LIT_BITS, false, c.len_lit, c.code_lit, lane, n_lanes, sync);
    build_code(c, c.freq_dist, N_DIST, LIT_BITS, false, c.len_dist, c.code_dist, lane, n_lanes, sync);
    if (lane == 0) rle_lengths(c);
    build_code(c, c.freq_bl, N_BL, BL_BITS, true, c.len_bl, c.code_bl, lane, n_lanes, sync);
    if (lane == 0) {
        uint32_t hclen = N_BL;
        while (hclen > 4 && c.len_bl[bl_order(hclen - 1)] == 0) --hclen;
        c.hclen = hclen;
        uint64_t fixed = 3, dyn = 3 + 5 + 5 + 4 + 3 * (uint64_t)hclen;
        for (uint32_t s = 0; s < N_BL; ++s) dyn += (uint64_t)c.freq_bl[s] * (c.len_bl[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u));
        for (uint32_t s = 0; s < N_LIT; ++s) {
            const uint32_t e = s > EOB ? len_ebits(s) : 0u;
            fixed += (uint64_t)c.freq_lit[s] * (fixed_len(s) + e);
            dyn += (uint64_t)c.freq_lit[s] * (c.len_lit[s] + e);
        }
        for (uint32_t s = 0; s < N_DIST; ++s) {
            fixed += (uint64_t)c.freq_dist[s] * (5 + dist_ebits(s));
            dyn += (uint64_t)c.freq_dist[s] * (c.len_dist[s] + dist_ebits(s));
        }
        c.bits[KIND_STORED] = 8 * (5 + n_text);
        c.bits[KIND_FIXED] = (uint32_t)fixed;      // (below 2^24: at most 65280 tokens of at most 48 bits)
        c.bits[KIND_DYNAMIC] = (uint32_t)dyn;
        uint32_t kind = KIND_STORED;
        if ((c.bits[KIND_FIXED] + 7) / 8 < (c.bits[kind] + 7) / 8) kind = KIND_FIXED;
        if ((c.bits[KIND_DYNAMIC] + 7) / 8 < (c.bits[kind] + 7) / 8) kind = KIND_DYNAMIC;
        c.kind = kind;
    }
    sync();
}
PF_DEF_HD inline uint32_t member_bytes(const Codes &c) { return HEADER + (c.bits[c.kind] + 7) / 8 + TRAILER; }

// a fixed block's codes in the place of the dynamic ones (shared)
template <typename Sync>
PF_DEF_HD inline void fixed_codes(Codes &c, uint32_t lane, uint32_t n_lanes, const Sync &sync) {
    sync();
    for (uint32_t s = lane; s < N_LIT; s += n_lanes) {
        const uint32_t l = fixed_len(s);
        const uint32_t code = s < 144 ? 0x30 + s : s < 256 ? 0x190 + (s - 144) : s < 280 ? s - 256 : 0xc0 + (s - 280);
        c.len_lit[s] = (uint8_t)l;
        c.code_lit[s] = (uint16_t)bit_reverse(code, l);
    }
    for (uint32_t s = lane; s < N_DIST; s += n_lanes) { c.len_dist[s] = 5; c.code_dist[s] = (uint16_t)bit_reverse(s, 5); }
    sync();
}

// ---- the member's bits ----
// the container's header and the block's (lane 0's work); returns the bit at which the tokens start.  For a stored block: LEN and NLEN
// too, and the text follows as bytes.
template <typename Out>
PF_DEF_HD inline uint32_t put_headers(const Codes &c, uint32_t n_text, Out &out) {
    const uint32_t bsize = member_bytes(c) - 1;
    out.put(0, 0x00000004088b1full, 64 - 8);                         // 1f 8b 08 04, MTIME (three bytes of it)
    out.put(56, 0xff00ull << 8 | 0x06ull << 24, 40);                 // MTIME's last, XFL, OS ff, XLEN = 6
    out.put(96, 0x00024342ull | ((uint64_t)bsize << 32), 48);        // 'B' 'C' 02 00 BSIZE - 1
    uint32_t at = HEADER * 8;
    out.put(at, 1u | (c.kind << 1), 3);
    at += 3;
    if (c.kind == KIND_STORED) {
        at = HEADER * 8 + 8;
        out.put(at, (uint64_t)n_text | ((uint64_t)(~n_text & 0xffffu) << 16), 32);
        return at + 32;
    }
    if (c.kind == KIND_FIXED) return at;
    out.put(at, (c.hlit - 257) | ((c.hdist - 1) << 5) | ((c.hclen - 4) << 10), 14);
    at += 14;
    for (uint32_t i = 0; i < c.hclen; ++i, at += 3) out.put(at, c.len_bl[bl_order(i)], 3);
    for (uint32_t i = 0; i < c.n_rle; ++i) {
        const uint32_t s = c.rle[i] & 31u, extra = c.rle[i] >> 5, l = c.len_bl[s];
        const uint32_t eb = s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u;
        out.put(at, (uint64_t)c.code_bl[s] | ((uint64_t)extra << l), l + eb);
        at += l + eb;
    }
    return at;
}

// one token's bits: *value, returns their number (at most 48)
PF_DEF_HD inline uint32_t literal_bits(const Codes &c, uint32_t byte, uint64_t *value) {
    *value = c.code_lit[byte];
    return c.len_lit[byte];
}
PF_DEF_HD inline uint32_t match_bits(const Codes &c, uint32_t len, uint32_t dist, uint64_t *value) {
    const Sym ls = len_sym(len), ds = dist_sym(dist);
    uint64_t v = c.code_lit[ls.sym];
    uint32_t n = c.len_lit[ls.sym];
    v |= (uint64_t)ls.extra << n;
    n += ls.ebits;
    v |= (uint64_t)c.code_dist[ds.sym] << n;
    n += c.len_dist[ds.sym];
    v |= (uint64_t)ds.extra << n;
    n += ds.ebits;
    *value = v;
    return n;
}
// the end-of-block code at `at` (the tokens' end) and the trailer (lane 0's work)
template <typename Out>
PF_DEF_HD inline void put_end(const Codes &c, uint32_t at, uint32_t crc, uint32_t n_text, Out &out) {
    if (c.kind != KIND_STORED) out.put(at, c.code_lit[EOB], c.len_lit[EOB]);
    const uint32_t t = (member_bytes(c) - TRAILER) * 8;
    out.put(t, crc, 32);
    out.put(t + 32, n_text, 32);
}

}  // namespace pf_deflate
