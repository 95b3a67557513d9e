// The deflate decoder that one lane executes, for both gzip readers and for kernel and host rule alike: K-INFLATE (pf_inflate.hip,
// pf_inflate_rule.hpp) drives it over one BGZF member (inflate_stream below), K-GUNZIP (pf_gunzip.hip, pf_gunzip_rule.hpp) over one piece
// of a plain gzip stream (pf_gunzip_core.hpp: decode_piece).  Here are the clause enum, the BGZF member header, the bit reader, the
// code tables from code lengths, the symbol loop (inflate_codes) and the block step (inflate_block) with every bounds test, and the
// CRC-32 pieces.  Nothing here allocates, and nothing here touches memory but through the three policies:
//   In     byte(i): compressed byte i of the payload for i < n_in (the reader never asks for another); raw(i): the same byte for a
//          stored block's copy, which every lane reads at a place of its own;
//   Sink   where the text goes and what bounds it (described in front of inflate_codes);
//   Work   the tables of one block (LDS on the device, the stack on the host).
// lane / n_lanes: the caller's place among those that execute the same call together (host: 0 of 1; kernel: a wavefront's 64 lanes,
// all with the same arguments).  What is serial is done by every lane alike; the table fill is shared.
//
// Every loop ends whatever the bytes say: the block loop consumes at least three bits a turn, the symbol loop consumes a bit or emits
// a byte a turn, a code is at most 15 bits, the code lengths are at most 320, and a reader past its last bit (`over`) ends them all.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PF_INF_HD __host__ __device__
#else
#define PF_INF_HD
#endif

namespace pf_inflate {

constexpr uint32_t MAX_ISIZE = 65536;    // a BGZF member inflates to at most 64 KiB
constexpr uint32_t HEADER_MIN = 18;      // 12 fixed bytes and the six of the BC subfield
constexpr uint32_t TRAILER = 8;          // CRC32, ISIZE
constexpr int FAST_BITS = 9;             // codes up to this length are decoded by one look-up
constexpr uint32_t MAX_LIT = 288, MAX_LENS = 320;

enum Clause {
    CLAUSE_NONE = 0,
    // ---- container ----
    CLAUSE_MAGIC,          // a member that does not start with 1f 8b
    CLAUSE_NOT_BLOCKED,    // gzip without a BC subfield: one deflate stream
    CLAUSE_METHOD,         // CM other than 8
    CLAUSE_FLAGS,          // flags other than FEXTRA
    CLAUSE_SHORT,          // a member shorter than its header and trailer
    CLAUSE_PAST_END,       // a member running past the end of the file
    CLAUSE_ISIZE,          // ISIZE above 65536
    // ---- stream ----
    CLAUSE_BTYPE3,
    CLAUSE_STORED_LEN,     // LEN / NLEN mismatch
    CLAUSE_STORED_PAST,    // a stored block running past the payload
    CLAUSE_TOO_MANY_CODES, // HLIT above 286 or HDIST above 30
    CLAUSE_CODE_LENGTHS,   // over-subscribed or incomplete code lengths
    CLAUSE_REPEAT,         // a repeat code with nothing to repeat, or running past HLIT + HDIST
    CLAUSE_NO_EOB,         // no end-of-block code
    CLAUSE_BAD_CODE,       // bits that are no code of an incomplete set
    CLAUSE_LITLEN_SYM,     // literal/length symbol 286 or 287
    CLAUSE_DIST_SYM,       // distance symbol 30 or 31
    CLAUSE_DIST_BEFORE,    // a distance reaching before the member's first byte
    CLAUSE_OUT_BEYOND,     // output beyond ISIZE
    CLAUSE_END,            // the final block ending anywhere but at the trailer
    CLAUSE_LENGTH,         // inflated length other than ISIZE
    CLAUSE_CRC,            // CRC-32 mismatch
    CLAUSE_COUNT_
};

struct Header {
    uint32_t payload_off;   // 12 + XLEN
    uint32_t member_len;    // BSIZE + 1
    uint32_t crc, isize;    // the trailer (read only when the member lies within the n bytes given)
};
struct Blocks { uint32_t stored, fixed, dynamic; };

// ---- container: one member header at p[0, n).  n = bytes from the member's start to the end of the file (or of the chunk) ----
template <typename Bytes>
PF_INF_HD inline int parse_member_bytes(const Bytes &p, uint64_t n, Header &h) {
    h = Header{0, 0, 0, 0};
    if (n < 2 || p[0] != 0x1f || p[1] != 0x8b) return CLAUSE_MAGIC;
    if (n < 4) return CLAUSE_PAST_END;
    if (p[2] != 8) return CLAUSE_METHOD;
    if (p[3] != 4) return CLAUSE_FLAGS;
    if (n < 12) return CLAUSE_PAST_END;
    const uint32_t xlen = (uint32_t)p[10] | ((uint32_t)p[11] << 8);
    if (n < 12 + (uint64_t)xlen) return CLAUSE_PAST_END;
    bool found = false;
    uint32_t bsize = 0;
    for (uint32_t at = 0; at + 4 <= xlen;) {   // (each turn moves on by at least four bytes)
        const uint32_t slen = (uint32_t)p[12 + at + 2] | ((uint32_t)p[12 + at + 3] << 8);
        if (at + 4 + slen > xlen) break;
        if (!found && p[12 + at] == 'B' && p[12 + at + 1] == 'C' && slen == 2) {
            bsize = (uint32_t)p[12 + at + 4] | ((uint32_t)p[12 + at + 5] << 8);
            found = true;
        }
        at += 4 + slen;
    }
    if (!found) return CLAUSE_NOT_BLOCKED;
    h.payload_off = 12 + xlen;
    h.member_len = bsize + 1;
    if (h.member_len < h.payload_off + TRAILER) return CLAUSE_SHORT;
    if ((uint64_t)h.member_len > n) return CLAUSE_PAST_END;
    const uint32_t t = h.member_len - TRAILER;
    h.crc = (uint32_t)p[t] | ((uint32_t)p[t + 1] << 8) | ((uint32_t)p[t + 2] << 16) | ((uint32_t)p[t + 3] << 24);
    h.isize = (uint32_t)p[t + 4] | ((uint32_t)p[t + 5] << 8) | ((uint32_t)p[t + 6] << 16) | ((uint32_t)p[t + 7] << 24);
    if (h.isize > MAX_ISIZE) return CLAUSE_ISIZE;
    return CLAUSE_NONE;
}

// ---- CRC-32 (reflected, polynomial edb88320), bit by bit: no table to place ----
constexpr uint32_t CRC_POLY = 0xedb88320u;
PF_INF_HD inline uint32_t crc_byte(uint32_t reg, uint32_t byte) {
    reg ^= byte;
    for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ (CRC_POLY & (0u - (reg & 1u)));
    return reg;
}
// a(x) * b(x) mod P, bit 31 = x^0
PF_INF_HD inline uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
// x^(8 * n_bytes) mod P
PF_INF_HD inline uint32_t crc_x8n(uint64_t n_bytes) {
    uint32_t p = 1u << 31, sq = 1u << 23;   // x^0, x^8
    for (; n_bytes; n_bytes >>= 1) {
        if (n_bytes & 1) p = crc_mul(sq, p);
        sq = crc_mul(sq, sq);
    }
    return p;
}
// The register after a slice, from zero and without the final inversion: linear in the bytes, so the registers of slices add up once
// each is moved on by the bytes behind it.
template <typename Bytes>
PF_INF_HD inline uint32_t crc_raw(const Bytes &p, uint32_t begin, uint32_t end) {
    uint32_t reg = 0;
    for (uint32_t i = begin; i < end; ++i) reg = crc_byte(reg, p[i]);
    return reg;
}
// bytes [0, n) cut into n_lanes slices of `slice_len(n, n_lanes)` bytes that end at n: the first slices may be empty, which a raw
// register does not see.  Slice j covers [slice_begin, slice_end); its register times slice_factor is its share of the whole.
PF_INF_HD inline uint32_t slice_len(uint32_t n, uint32_t n_lanes) { return (n + n_lanes - 1) / n_lanes; }
PF_INF_HD inline uint32_t slice_end(uint32_t n, uint32_t n_lanes, uint32_t j) {
    const uint64_t back = (uint64_t)slice_len(n, n_lanes) * (n_lanes - 1 - j);
    return back >= n ? 0 : n - (uint32_t)back;
}
PF_INF_HD inline uint32_t slice_begin(uint32_t n, uint32_t n_lanes, uint32_t j) { return j == 0 ? 0 : slice_end(n, n_lanes, j - 1); }
PF_INF_HD inline uint32_t slice_share(uint32_t raw, uint32_t n, uint32_t n_lanes, uint32_t j) {
    return crc_mul(crc_x8n((uint64_t)slice_len(n, n_lanes) * (n_lanes - 1 - j)), raw);
}
// the CRC-32 of n bytes from the sum (xor) of the shares: the initial ffffffff moved on by n bytes, and the final inversion
PF_INF_HD inline uint32_t crc_finish(uint32_t raw_sum, uint64_t n) { return raw_sum ^ crc_mul(crc_x8n(n), 0xffffffffu) ^ 0xffffffffu; }

// ---- the bit reader: bytes are fetched only when a bit of them is needed, and never beyond n_in ----
template <typename In>
struct BitReader {
    const In &in;
    uint32_t n_in;
    uint32_t pos = 0;    // bytes fetched (may count past n_in: those are zeros that were never read)
    uint32_t buf = 0;
    int cnt = 0;         // bits held
    bool over = false;   // bits beyond the payload have been consumed
    PF_INF_HD BitReader(const In &i, uint32_t n) : in(i), n_in(n) {}
    PF_INF_HD void need(int n) {   // n <= 16
        while (cnt < n) {
            const uint32_t b = pos < n_in ? (uint32_t)in.byte(pos) : 0u;
            buf |= b << cnt;
            ++pos;
            cnt += 8;
        }
    }
    PF_INF_HD uint32_t peek(int n) { need(n); return buf & ((1u << n) - 1u); }
    PF_INF_HD void drop(int n) {
        buf >>= n;
        cnt -= n;
        if ((uint64_t)pos * 8 - (uint64_t)cnt > (uint64_t)n_in * 8) over = true;
    }
    PF_INF_HD uint32_t bits(int n) { const uint32_t v = peek(n); drop(n); return v; }
    // to the next byte boundary; the whole bytes still held are given back.  Returns the byte position.
    PF_INF_HD uint32_t align() {
        drop(cnt & 7);
        pos -= (uint32_t)(cnt >> 3);
        cnt = 0;
        buf = 0;
        return pos;
    }
    PF_INF_HD uint32_t bytes_consumed() const { return (uint32_t)(((uint64_t)pos * 8 - (uint64_t)cnt + 7) / 8); }
};

// ---- code tables ----
struct Huff {
    uint16_t count[16];          // codes of each length
    uint16_t first[16];          // the first code of each length
    uint16_t start[16];          // where the symbols of each length begin in symbol[]
    uint16_t symbol[MAX_LIT];    // symbols in the order of their codes
    uint16_t fast[1 << FAST_BITS];   // by the next FAST_BITS bits: symbol << 4 | length, 0 = a longer code (or none)
};
struct Work {
    Huff lit, dist;
    uint16_t lengths[MAX_LENS];
};

// what a caller of several lanes puts between the writes of some and the reads of others (host: nothing)
struct NoSync { PF_INF_HD void operator()() const {} };

PF_INF_HD inline uint32_t bit_reverse(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) { r = (r << 1) | (code & 1u); code >>= 1; }
    return r;
}

// lengths[0, n) -> h.  Returns what is left of the code space: 0 complete, > 0 incomplete, < 0 over-subscribed (h is then not usable).
template <typename Sync>
PF_INF_HD inline int build_huff(Huff &h, const uint16_t *lengths, uint32_t n, uint32_t lane, uint32_t n_lanes, const Sync &sync) {
    sync();   // (the lengths, and whoever still reads the last table)
    // serial, by every lane alike (the same values to the same places)
    for (int l = 0; l < 16; ++l) h.count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) h.count[lengths[s] & 15] = (uint16_t)(h.count[lengths[s] & 15] + 1);
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= (int)h.count[l];
        if (left < 0) return left;
    }
    uint32_t code = 0, at = 0;
    h.first[0] = 0;
    h.start[0] = 0;
    for (int l = 1; l < 16; ++l) {
        code = (code + (l > 1 ? (uint32_t)h.count[l - 1] : 0u)) << 1;
        h.first[l] = (uint16_t)code;
        h.start[l] = (uint16_t)at;
        at += h.count[l];
    }
    uint16_t *next = h.fast;   // (free until the look-up is filled below)
    for (int l = 0; l < 16; ++l) next[l] = h.start[l];
    for (uint32_t s = 0; s < n; ++s) {
        const int l = lengths[s] & 15;
        if (l) { h.symbol[next[l]] = (uint16_t)s; next[l] = (uint16_t)(next[l] + 1); }
    }
    sync();
    // shared: the look-up of the short codes
    for (uint32_t j = lane; j < (1u << FAST_BITS); j += n_lanes) h.fast[j] = 0;
    sync();
    for (uint32_t k = lane; k < at; k += n_lanes) {
        const uint32_t s = h.symbol[k];
        const int l = lengths[s] & 15;
        if (l > FAST_BITS) continue;
        const uint32_t c = bit_reverse((uint32_t)h.first[l] + (k - h.start[l]), l);
        for (uint32_t j = c; j < (1u << FAST_BITS); j += 1u << l) h.fast[j] = (uint16_t)((s << 4) | (uint32_t)l);
    }
    sync();
    return left;
}

// the next symbol, or -1 when the bits are no code of the set
template <typename In>
PF_INF_HD inline int decode_symbol(BitReader<In> &br, const Huff &h) {
    const uint32_t e = h.fast[br.peek(FAST_BITS)];
    if (e) { br.drop((int)(e & 15u)); return (int)(e >> 4); }
    uint32_t code = 0;
    for (int l = 1; l < 16; ++l) {
        code = (code << 1) | br.bits(1);
        const uint32_t c = h.count[l];
        if (c && code >= h.first[l] && code - h.first[l] < c) return (int)h.symbol[h.start[l] + (code - h.first[l])];
    }
    return -1;
}

// a set is usable when it is complete, or holds at most one code, of one bit (what a compressor writes for a single distance or none)
PF_INF_HD inline bool huff_usable(const Huff &h, int left, uint32_t n) {
    return left == 0 || (left > 0 && (uint32_t)h.count[0] + (uint32_t)h.count[1] == n);
}

template <typename In, typename Sync>
PF_INF_HD inline int read_dynamic(BitReader<In> &br, Work &w, uint32_t lane, uint32_t n_lanes, const Sync &sync) {
    const uint32_t nlen = br.bits(5) + 257, ndist = br.bits(5) + 1, ncode = br.bits(4) + 4;
    if (nlen > 286 || ndist > 30) return CLAUSE_TOO_MANY_CODES;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    sync();
    for (uint32_t i = 0; i < 19; ++i) w.lengths[order[i]] = (uint16_t)(i < ncode ? br.bits(3) : 0u);
    if (br.over) return CLAUSE_END;
    if (build_huff(w.dist, w.lengths, 19, lane, n_lanes, sync) != 0) return CLAUSE_CODE_LENGTHS;   // (w.dist lends its place to the 19 codes)
    // the table is built and no longer reads w.lengths: the lengths it decodes go there, by every lane alike
    uint32_t idx = 0;
    while (idx < nlen + ndist) {   // a turn consumes at least one bit
        const int sym = decode_symbol(br, w.dist);
        if (br.over) return CLAUSE_END;
        if (sym < 0) return CLAUSE_BAD_CODE;
        if (sym < 16) { w.lengths[idx++] = (uint16_t)sym; continue; }
        uint32_t val = 0, rep;
        if (sym == 16) {
            if (idx == 0) return CLAUSE_REPEAT;
            val = w.lengths[idx - 1];
            rep = 3 + br.bits(2);
        } else if (sym == 17) rep = 3 + br.bits(3);
        else rep = 11 + br.bits(7);
        if (idx + rep > nlen + ndist) return CLAUSE_REPEAT;
        while (rep--) w.lengths[idx++] = (uint16_t)val;
    }
    if (br.over) return CLAUSE_END;
    sync();
    if (w.lengths[256] == 0) return CLAUSE_NO_EOB;
    int left = build_huff(w.lit, w.lengths, nlen, lane, n_lanes, sync);
    if (!huff_usable(w.lit, left, nlen)) return CLAUSE_CODE_LENGTHS;
    left = build_huff(w.dist, w.lengths + nlen, ndist, lane, n_lanes, sync);
    if (!huff_usable(w.dist, left, ndist)) return CLAUSE_CODE_LENGTHS;
    return CLAUSE_NONE;
}

template <typename Sync>
PF_INF_HD inline void build_fixed(Work &w, uint32_t lane, uint32_t n_lanes, const Sync &sync) {
    sync();
    for (uint32_t s = lane; s < MAX_LIT; s += n_lanes) w.lengths[s] = (uint16_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (uint32_t s = lane; s < 32; s += n_lanes) w.lengths[MAX_LIT + s] = 5;   // all 32, so that 30 and 31 are refused by name
    (void)build_huff(w.lit, w.lengths, MAX_LIT, lane, n_lanes, sync);
    (void)build_huff(w.dist, w.lengths + MAX_LIT, 32, lane, n_lanes, sync);
}

// ---- the decoder: one symbol loop and one block step, for every caller, through a sink ----
// A Sink says where the text goes and what bounds it:
//   Pos                  the type of a place in the text: uint32_t for a BGZF member (K-INFLATE's arithmetic stays 32-bit), uint64_t for
//                        a piece of a plain gzip stream
//   BEYOND               the clause for text past the bound: CLAUSE_OUT_BEYOND for a member, pf_gunzip::CLAUSE_PIECE_LIMIT for a piece
//   reach()              bytes of text in front of place 0 that a distance may refer to (0 for a member)
//   put(at, byte), copy(at, distance, length), stored(in, src, at, length)
//                        called only after the tests below have passed: at + length <= bound, distance <= at + reach(),
//                        src + length <= n_in (stored reads the payload through in.raw)

// the symbols of one fixed or dynamic block; the four tables of RFC 1951, 3.2.5
template <typename In, typename Sink>
PF_INF_HD inline int inflate_codes(BitReader<In> &br, const Work &w, Sink &sink, typename Sink::Pos &at, typename Sink::Pos bound) {
    typedef typename Sink::Pos Pos;
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    for (;;) {   // a turn consumes at least one bit
        int sym = decode_symbol(br, w.lit);
        if (br.over) return CLAUSE_END;   // (bits that are not there decide nothing)
        if (sym < 0) return CLAUSE_BAD_CODE;
        if (sym < 256) {
            if (at >= bound) return Sink::BEYOND;
            sink.put(at, (uint8_t)sym);
            ++at;
            continue;
        }
        if (sym == 256) return CLAUSE_NONE;
        sym -= 257;
        if (sym >= 29) return CLAUSE_LITLEN_SYM;
        const uint32_t len = (uint32_t)lbase[sym] + br.bits(lext[sym]);
        const int ds = decode_symbol(br, w.dist);
        if (br.over) return CLAUSE_END;
        if (ds < 0) return CLAUSE_BAD_CODE;
        if (ds >= 30) return CLAUSE_DIST_SYM;
        const uint32_t dist = (uint32_t)dbase[ds] + br.bits(dext[ds]);
        if (br.over) return CLAUSE_END;
        if ((Pos)dist > at && (Pos)dist - at > sink.reach()) return CLAUSE_DIST_BEFORE;
        if ((Pos)len > bound - at) return Sink::BEYOND;
        sink.copy(at, dist, len);
        at += len;
    }
}

// One block from its BFINAL bit on: its text through the sink, `at` moved on, its kind counted, *last = BFINAL.  Returns the clause;
// the two of them that say where the bits ran out are the caller's to judge: CLAUSE_END (at the header or inside the block) and
// CLAUSE_STORED_PAST (a stored block past the payload).
template <typename In, typename Sink, typename Sync>
PF_INF_HD inline int inflate_block(BitReader<In> &br, const In &in, uint32_t n_in, Sink &sink, typename Sink::Pos &at, typename Sink::Pos bound, Work &w,
                                   uint32_t lane, uint32_t n_lanes, const Sync &sync, Blocks &blocks, uint32_t &last) {
    typedef typename Sink::Pos Pos;
    last = br.bits(1);
    const uint32_t type = br.bits(2);
    if (br.over) return CLAUSE_END;
    if (type == 0) {
        const uint32_t p0 = br.align();
        if (br.over || (uint64_t)p0 + 4 > n_in) return CLAUSE_STORED_PAST;
        const uint32_t len = br.bits(16), nlen = br.bits(16);
        if (len != (~nlen & 0xffffu)) return CLAUSE_STORED_LEN;
        const uint32_t src = br.align();
        if (len > n_in - src) return CLAUSE_STORED_PAST;
        if ((Pos)len > bound - at) return Sink::BEYOND;
        sink.stored(in, src, at, len);
        br.pos = src + len;
        at += len;
        ++blocks.stored;
        return CLAUSE_NONE;
    }
    if (type == 1) {
        build_fixed(w, lane, n_lanes, sync);
        ++blocks.fixed;
        return inflate_codes(br, w, sink, at, bound);
    }
    if (type == 2) {
        const int clause = read_dynamic(br, w, lane, n_lanes, sync);
        ++blocks.dynamic;
        return clause ? clause : inflate_codes(br, w, sink, at, bound);
    }
    return CLAUSE_BTYPE3;
}

// One member's deflate stream: n_in payload bytes -> exactly isize bytes.  *produced = bytes written (<= isize on every path).
template <typename In, typename Out, typename Sync>
PF_INF_HD inline int inflate_stream(const In &in, uint32_t n_in, Out &out, uint32_t isize, Work &w, uint32_t lane, uint32_t n_lanes, const Sync &sync,
                                    Blocks &blocks, uint32_t &produced) {
    BitReader<In> br(in, n_in);
    uint32_t at = 0;
    blocks = Blocks{0, 0, 0};
    produced = 0;
    int clause = CLAUSE_NONE;
    for (;;) {   // a turn consumes at least three bits
        uint32_t last = 0;
        clause = inflate_block(br, in, n_in, out, at, isize, w, lane, n_lanes, sync, blocks, last);
        if (clause || last) break;
    }
    produced = at;
    if (clause) return clause;
    if (br.over || br.bytes_consumed() != n_in) return CLAUSE_END;
    if (at != isize) return CLAUSE_LENGTH;
    return CLAUSE_NONE;
}

}  // namespace pf_inflate
