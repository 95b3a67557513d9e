// The part of K-GUNZIP that one lane executes, for the kernel (pf_gunzip.hip) and the host rule (pf_gunzip_rule.hpp) alike.  Plain gzip
// is one deflate stream per member: its blocks start at unknown bits and reach 32 KiB back.  It is made parallel in pieces:
//   block_candidate   does a non-final dynamic block header start at this bit?  (the search for piece starts; a hint, never trusted)
//   decode_piece      the blocks from a start bit on, through a Sink, until a final block, a piece start it lands on, the end of the
//                     bits (the last complete block boundary is kept: "tail") or a clause
//   CountSink         produces nothing: the first pass, which gives every piece its end, its link and its number of symbols
//   RingSink          16-bit symbols through a ring of the last 32 Ki symbols: a byte is 0..255, a back-reference that reaches in front
//                     of the piece is the marker 0x8000 | (32768 + at - dist), an index into the 32 KiB in front of the piece
//   behind            the byte a marker stands for, for the window and resolve stages
// The decoder itself -- the bit reader, the code tables, the symbol loop and the block step -- is pf_inflate_core.hpp's, the one K-INFLATE
// runs: decode_piece is a loop around pf_inflate::inflate_block, and a piece's sinks say what differs (64-bit places, text in front of
// place 0, CLAUSE_PIECE_LIMIT for text past the bound).
//
// Every loop ends whatever the bytes say: the block loop consumes at least three bits a turn, the symbol loop a bit or a symbol, and a
// reader past its last bit ends them all.  Nothing is read outside in[0, n_bytes), and a RingSink writes stage[0, max_syms) only.
#pragma once
#include "pf_inflate_core.hpp"

namespace pf_gunzip {

using pf_inflate::BitReader;
using pf_inflate::Blocks;
using pf_inflate::Huff;
using pf_inflate::Work;

constexpr uint32_t RING = 32768, RING_MASK = RING - 1;   // symbols a back-reference can reach
constexpr uint32_t FLUSH = 8192;                         // symbols the ring holds at most before they go to the staging array
constexpr uint32_t PIECE_DEFAULT = 16384, PIECE_MIN = 64;
constexpr uint16_t MARKER = 0x8000;
constexpr uint16_t RESOLVED = 0x4000;   // in the staging array only: a marker the window stage has replaced by its byte (bit 15 clear)

// clauses of plain gzip, numbered behind pf_inflate's (whose stream clauses are used as they are)
enum Clause {
    CLAUSE_RESERVED_FLAG = pf_inflate::CLAUSE_COUNT_,   // a reserved FLG bit
    CLAUSE_HEADER_PAST,     // a member header running past the end of the file
    CLAUSE_CUT_BLOCK,       // the file ends inside a deflate block
    CLAUSE_CUT_TRAILER,     // the file ends inside CRC32 / ISIZE
    CLAUSE_TRAILING,        // bytes behind a trailer that start no gzip member
    CLAUSE_BLOCK_TOO_LARGE, // a deflate block of more compressed bytes than the carry holds
    CLAUSE_PIECE_LIMIT,     // (internal) the second pass of a piece differs from its first
    CLAUSE_END_
};

constexpr uint32_t LINK_TAIL = 0xffffffffu;    // the bits ran out inside a block: end_bit is the last complete boundary
constexpr uint32_t LINK_FINAL = 0xfffffffeu;   // the last block was final
constexpr uint32_t LINK_CLAUSE = 0xfffffffdu;  // refused: clause, and end_bit is the last complete boundary
constexpr uint32_t LINK_LIMIT = 0xfffffffcu;   // the second pass reached the end bit the first one gave
constexpr uint64_t NO_BIT = ~0ull;

struct Piece {
    uint64_t end_bit;    // the last complete block boundary
    uint64_t symbols;    // bytes of text up to it
    uint32_t link;       // the piece start landed on, or LINK_*
    uint32_t clause;
    uint32_t stored, fixed, dynamic;   // complete blocks
    uint32_t pad_;
};

// ---- the search: a non-final dynamic block header at `bit`?  Registers and small private arrays only ----
template <typename Bytes>
struct CandBits {
    const Bytes &p;
    uint64_t n_bytes, pos;
    bool over;
    PF_INF_HD uint32_t get(int n) {   // n <= 16
        if (pos + (uint64_t)n > n_bytes * 8) { over = true; return 0; }
        const uint64_t i = pos >> 3;
        uint32_t w = (uint32_t)p[i];
        if (i + 1 < n_bytes) w |= (uint32_t)p[i + 1] << 8;
        if (i + 2 < n_bytes) w |= (uint32_t)p[i + 2] << 16;
        const uint32_t v = (w >> (pos & 7)) & ((1u << n) - 1u);
        pos += (uint64_t)n;
        return v;
    }
};

template <typename Bytes>
PF_INF_HD inline bool block_candidate(const Bytes &p, uint64_t n_bytes, uint64_t bit) {
    CandBits<Bytes> b{p, n_bytes, bit, false};
    if (b.get(3) != 4u || b.over) return false;   // BFINAL 0, BTYPE 2
    const uint32_t nlen = b.get(5) + 257, ndist = b.get(5) + 1, ncode = b.get(4) + 4;
    if (b.over || nlen > 286 || ndist > 30) return false;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) cl[order[i]] = (uint8_t)b.get(3);
    if (b.over) return false;
    // the code-length code: complete, then canonical
    uint8_t count[8], start[8], next[8], symbol[19];
    uint16_t first[8];
    for (int l = 0; l < 8; ++l) count[l] = 0;
    for (int s = 0; s < 19; ++s) ++count[cl[s]];
    int left = 1;
    for (int l = 1; l < 8; ++l) {
        left = (left << 1) - (int)count[l];
        if (left < 0) return false;
    }
    if (left != 0) return false;
    uint32_t code = 0, at = 0;
    first[0] = 0;
    start[0] = next[0] = 0;
    for (int l = 1; l < 8; ++l) {
        code = (code + (l > 1 ? (uint32_t)count[l - 1] : 0u)) << 1;
        first[l] = (uint16_t)code;
        start[l] = next[l] = (uint8_t)at;
        at += count[l];
    }
    for (int s = 0; s < 19; ++s)
        if (cl[s]) symbol[next[cl[s]]++] = (uint8_t)s;
    // HLIT + HDIST lengths: only their counts per length and the end-of-block code are kept
    uint16_t litc[16], distc[16];
    for (int l = 0; l < 16; ++l) litc[l] = distc[l] = 0;
    bool eob = false;
    uint32_t idx = 0, prev = 0;
    const uint32_t total = nlen + ndist;
    while (idx < total) {   // a turn adds at least one length
        uint32_t c = 0;
        int sym = -1;
        for (int l = 1; l < 8; ++l) {
            c = (c << 1) | b.get(1);
            if (count[l] && c >= first[l] && c - first[l] < count[l]) { sym = symbol[start[l] + (c - first[l])]; break; }
        }
        if (b.over || sym < 0) return false;
        uint32_t len, rep = 1;
        if (sym < 16) len = (uint32_t)sym;
        else if (sym == 16) {
            if (idx == 0) return false;
            len = prev;
            rep = 3 + b.get(2);
        } else if (sym == 17) { len = 0; rep = 3 + b.get(3); }
        else { len = 0; rep = 11 + b.get(7); }
        if (b.over || idx + rep > total) return false;
        for (; rep; --rep, ++idx) {
            if (idx < nlen) { ++litc[len]; if (idx == 256 && len) eob = true; }
            else ++distc[len];
        }
        prev = len;
    }
    if (!eob) return false;
    left = 1;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - (int)litc[l];
        if (left < 0) return false;
    }
    if (left != 0) return false;   // a complete literal/length set
    left = 1;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - (int)distc[l];
        if (left < 0) return false;
    }
    return left == 0 || (uint32_t)distc[0] + (uint32_t)distc[1] == ndist;   // a usable distance set (pf_inflate::huff_usable)
}

// ---- sinks ----
struct CountSink {
    typedef uint64_t Pos;
    static constexpr int BEYOND = CLAUSE_PIECE_LIMIT;
    PF_INF_HD uint64_t reach() const { return ~0ull; }   // (what lies in front of a piece is known to the second pass only)
    PF_INF_HD void put(uint64_t, uint32_t) {}
    PF_INF_HD void copy(uint64_t, uint32_t, uint32_t) {}
    template <typename In>
    PF_INF_HD void stored(const In &, uint32_t, uint64_t, uint32_t) {}
    PF_INF_HD void finish(uint64_t) {}
};

// ring[RING] is shared by the n_lanes callers (LDS on the device); stage is the piece's range of the staging array.  The core has
// tested every range: at + len <= max_syms, and dist <= at + before.
template <typename Sync>
struct RingSink {
    typedef uint64_t Pos;
    static constexpr int BEYOND = CLAUSE_PIECE_LIMIT;
    uint16_t *ring, *stage;
    uint64_t before;        // bytes of text in front of the piece (earlier pieces of the call and the window)
    uint32_t lane, n_lanes;
    Sync sync;
    uint64_t flushed = 0;   // symbols [0, flushed) of the piece are in the staging array
    PF_INF_HD RingSink(uint16_t *r, uint16_t *s, uint64_t b, uint32_t l, uint32_t n, const Sync &sy) : ring(r), stage(s), before(b), lane(l), n_lanes(n), sync(sy) {}
    PF_INF_HD uint64_t reach() const { return before; }
    PF_INF_HD void flush(uint64_t upto) {   // upto - flushed <= RING
        sync();
        for (uint64_t i = flushed + lane; i < upto; i += n_lanes) stage[i] = ring[i & RING_MASK];
        flushed = upto;
        sync();
    }
    PF_INF_HD void put(uint64_t at, uint32_t byte) {
        if (lane == 0) ring[at & RING_MASK] = (uint16_t)byte;
        if (at + 1 - flushed >= FLUSH) flush(at + 1);
    }
    PF_INF_HD void copy(uint64_t at, uint32_t dist, uint32_t len) {   // len <= 258, dist <= 32768
        sync();   // the symbols in front of `at` are in place
        for (uint32_t i = lane; i < len; i += n_lanes) {
            const uint32_t j = dist >= len ? i : i % dist;   // (a distance below the length repeats the pattern)
            uint16_t v;
            if (at + j < (uint64_t)dist) v = (uint16_t)(MARKER | (uint32_t)(RING + at + j - dist));
            else v = ring[(at + j - dist) & RING_MASK];
            ring[(at + i) & RING_MASK] = v;
        }
        if (at + len - flushed >= FLUSH) flush(at + len);
    }
    template <typename In>
    PF_INF_HD void stored(const In &in, uint32_t src, uint64_t at, uint32_t len) {   // src + len <= n_bytes
        for (uint32_t done = 0; done < len;) {
            const uint32_t n = len - done < FLUSH ? len - done : FLUSH;
            for (uint32_t i = lane; i < n; i += n_lanes) ring[(at + done + i) & RING_MASK] = (uint16_t)in.raw(src + done + i);
            done += n;
            if (at + done - flushed >= FLUSH) flush(at + done);
        }
    }
    PF_INF_HD void finish(uint64_t at) { if (at > flushed) flush(at); }
};

template <typename In>
PF_INF_HD inline uint64_t bit_pos(const BitReader<In> &br) { return (uint64_t)br.pos * 8 - (uint64_t)br.cnt; }

// Blocks of in[0, n_bytes) from start_bit on (start_bit <= 8 * n_bytes).  stops[0, n_stops) are the piece starts, ascending; next_stop is
// the first that may stop this piece (stops = nullptr: none does).  limit_bit / max_syms: the second pass stops at the boundary the
// first one recorded and makes no more symbols than it counted (first pass: NO_BIT, ~0).
template <typename In, typename Sink, typename Sync>
PF_INF_HD inline void decode_piece(const In &in, uint32_t n_bytes, uint64_t start_bit, const uint64_t *stops, uint32_t n_stops, uint32_t next_stop,
                                   uint64_t limit_bit, uint64_t max_syms, Sink &sink, Work &w, uint32_t lane, uint32_t n_lanes, const Sync &sync, Piece &r) {
    BitReader<In> br(in, n_bytes);
    br.pos = (uint32_t)(start_bit >> 3);
    if (start_bit & 7) (void)br.bits((int)(start_bit & 7));
    r = Piece{start_bit, 0, LINK_TAIL, 0, 0, 0, 0, 0};
    uint64_t at = 0;
    Blocks blk{0, 0, 0};
    uint32_t k = next_stop;
    if (start_bit >= limit_bit) r.link = LINK_LIMIT;   // (a piece without a complete block)
    else for (;;) {   // a turn consumes at least three bits
        uint32_t last = 0;
        const int clause = pf_inflate::inflate_block(br, in, n_bytes, sink, at, max_syms, w, lane, n_lanes, sync, blk, last);
        if (clause == pf_inflate::CLAUSE_END || clause == pf_inflate::CLAUSE_STORED_PAST) break;   // the bits ran out at or inside the block: tail
        if (clause) { r.clause = (uint32_t)clause; r.link = LINK_CLAUSE; break; }
        r.end_bit = bit_pos(br);
        r.symbols = at;
        r.stored = blk.stored;
        r.fixed = blk.fixed;
        r.dynamic = blk.dynamic;
        if (r.end_bit >= limit_bit) { r.link = LINK_LIMIT; break; }
        if (last) { r.link = LINK_FINAL; break; }
        if (stops) {
            while (k < n_stops && stops[k] < r.end_bit) ++k;   // a start that has been passed is skipped for good
            if (k < n_stops && stops[k] == r.end_bit) { r.link = k; break; }
        }
    }
    sink.finish(r.symbols);
}

// ---- the member's CRC from the calls' raw registers: (raw, len) of the text so far, then a call's (raw, len) behind it ----
PF_INF_HD inline uint32_t crc_append(uint32_t raw_so_far, uint32_t raw_next, uint64_t len_next) {
    return pf_inflate::crc_mul(pf_inflate::crc_x8n(len_next), raw_so_far) ^ raw_next;
}
// (the CRC-32 itself is pf_inflate::crc_finish of the last register and the member's length)

// ---- the byte a marker v of a piece at `place` stands for: from the staging array in front of the piece, or from the window[0, n_window)
// in front of the call (a marker that reaches in front of both was refused by the decode stage) ----
PF_INF_HD inline uint32_t behind(const uint16_t *stage, const uint8_t *window, uint32_t n_window, uint64_t place, uint32_t v) {
    const int64_t q = (int64_t)place - (int64_t)RING + (int64_t)(v & 0x7fffu);
    if (q >= 0) return (uint32_t)stage[q] & 0xffu;
    const int64_t wq = (int64_t)n_window + q;
    return wq >= 0 ? (uint32_t)window[wq] : 0u;
}

}  // namespace pf_gunzip
