// The rule of K-GUNZIP (plain gzip, `--gz-plain`) in one place, for the host layer (host/pf_gz_host.cpp), the kernel's error texts
// (pf_gunzip.hip) and the stand-alone test (tests/cpp/test_gunzip_rule.cpp).
//
// A gzip file (RFC 1952) is one or more members, each
//   1f 8b | CM = 8 | FLG | MTIME XFL OS | [XLEN, extra] [name 0] [comment 0] [CRC16] | a deflate stream (RFC 1951) | CRC32 | ISIZE
// with ISIZE the length mod 2^32.  The container is read on the host (gzip_header, Stream below); the deflate stream is inflated in
// pieces: inflate_call here runs the algorithm of pf_inflate_gzip (pf_gunzip.hip) as lane 0 of 1 over plain memory -- find, count,
// chain, decode, window, resolve, with the same core (pf_gunzip_core.hpp) -- so whatever keeps a corrupt stream inside its ranges is
// checked on the CPU.  Stream is the loop both streams (host/pf_reads_stream.hpp) run per gzip file: carry + block -> call -> text, trailer, next header.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "pf_gunzip_core.hpp"
#include "pf_inflate_rule.hpp"

namespace pf_gunzip {

constexpr uint64_t CARRY_MAX = 64ull << 20;   // compressed bytes held while no block in them is complete

inline const char *clause_text(int c) {
    switch (c) {
        case CLAUSE_RESERVED_FLAG: return "a reserved bit of the gzip flags is set";
        case CLAUSE_HEADER_PAST: return "the member's header runs past the end of the file";
        case CLAUSE_CUT_BLOCK: return "the file ends inside a deflate block";
        case CLAUSE_CUT_TRAILER: return "the file ends inside the member's trailer";
        case CLAUSE_TRAILING: return "bytes behind the trailer that start no gzip member";
        case CLAUSE_BLOCK_TOO_LARGE: return "a deflate block of more than 64 MiB of compressed bytes";
        case CLAUSE_PIECE_LIMIT: return "the two passes over a piece of the stream differ";
        case pf_inflate::CLAUSE_LENGTH: return "the inflated length differs from ISIZE mod 2^32";
        default: return pf_inflate::clause_text(c);
    }
}

// ---- container ----
// one member header at p[0, n).  0: *len = its bytes.  CLAUSE_HEADER_PAST: the n bytes end inside it (more may follow).
inline int gzip_header(const uint8_t *p, uint64_t n, uint64_t *len) {
    if (len) *len = 0;
    if (n >= 1 && p[0] != 0x1f) return pf_inflate::CLAUSE_MAGIC;
    if (n >= 2 && p[1] != 0x8b) return pf_inflate::CLAUSE_MAGIC;
    if (n >= 3 && p[2] != 8) return pf_inflate::CLAUSE_METHOD;
    if (n >= 4 && (p[3] & 0xe0)) return CLAUSE_RESERVED_FLAG;
    if (n < 10) return CLAUSE_HEADER_PAST;
    const uint32_t flg = p[3];
    uint64_t at = 10;
    if (flg & 4) {   // FEXTRA
        if (n < at + 2) return CLAUSE_HEADER_PAST;
        at += 2 + ((uint64_t)p[at] | ((uint64_t)p[at + 1] << 8));
        if (n < at) return CLAUSE_HEADER_PAST;
    }
    for (int field = 0; field < 2; ++field) {   // FNAME, FCOMMENT: to their zero
        if (!(flg & (field ? 16u : 8u))) continue;
        while (at < n && p[at]) ++at;
        if (at >= n) return CLAUSE_HEADER_PAST;
        ++at;
    }
    if (flg & 2) at += 2;   // FHCRC (not checked)
    if (n < at) return CLAUSE_HEADER_PAST;
    if (len) *len = at;
    return pf_inflate::CLAUSE_NONE;
}

// What the first bytes of a file say with `--gz-plain`: FILE_PLAIN (no magic), FILE_BGZF (FLG = 04 and a BC subfield: K-INFLATE, with
// its own refusals), FILE_GZIP, or FILE_REFUSED with *clause.
enum FileKind { FILE_PLAIN = 0, FILE_BGZF = 1, FILE_REFUSED = 2, FILE_GZIP = 3 };
inline int file_kind(const uint8_t *first, uint64_t n_first, uint64_t file_size, int *clause) {
    if (clause) *clause = 0;
    if (n_first < 2 || first[0] != 0x1f || first[1] != 0x8b) return FILE_PLAIN;
    if (n_first >= 4 && first[2] == 8 && first[3] == 4) {
        int c = 0;
        const int kind = pf_inflate::file_clause_gz(first, n_first, file_size, &c);
        if (c != pf_inflate::CLAUSE_NOT_BLOCKED) { if (clause) *clause = c; return kind; }
    }
    uint64_t len = 0;
    int c = gzip_header(first, n_first, &len);
    if (c == CLAUSE_HEADER_PAST && n_first < file_size) c = 0;   // (cut by the bytes looked at, not by the file: judged when the stream runs)
    if (clause) *clause = c;
    return c ? FILE_REFUSED : FILE_GZIP;
}

// ---- one call: the algorithm of pf_inflate_gzip over plain memory ----
struct Call {
    uint64_t out_bytes = 0, end_bit = 0;
    uint32_t final = 0;       // the call ended behind a final block
    uint32_t n_window = 0;    // bytes of the new window
    uint32_t crc_raw = 0;     // the raw CRC register of the call's text (crc_append)
    uint32_t clause = 0;
    uint64_t clause_bit = 0;
};
struct Stats {
    uint64_t pieces_found = 0, pieces_live = 0, pieces_dead = 0, markers = 0, blocks_stored = 0, blocks_fixed = 0, blocks_dynamic = 0, bytes_in = 0, bytes_out = 0;
};

using pf_inflate::HostIn;

inline uint32_t piece_stride(uint32_t piece_bytes) { return piece_bytes == 0 ? PIECE_DEFAULT : piece_bytes < PIECE_MIN ? PIECE_MIN : piece_bytes; }
// the first nominal boundary behind start_bit, and how many there are in front of the end of the bytes
inline uint64_t first_boundary(uint64_t start_bit, uint32_t stride) { return start_bit / 8 / stride + 1; }
inline uint64_t boundary_count(uint64_t n_bytes, uint64_t start_bit, uint32_t stride) {
    const uint64_t j0 = first_boundary(start_bit, stride), j1 = (n_bytes + stride - 1) / stride;   // boundaries j0 .. j1 - 1
    return j1 > j0 ? j1 - j0 : 0;
}

// window[0, n_window): the last bytes of the member's text so far; new_window holds 32768 bytes and may not overlap window.
// out is resized to the text of the call.  Reads comp[0, n_bytes) only.
inline void inflate_call(const uint8_t *comp, uint64_t n_bytes, uint64_t start_bit, const uint8_t *window, uint32_t n_window, uint32_t piece_bytes,
                         std::vector<uint8_t> &out, uint8_t *new_window, Call &res, Stats *stats = nullptr) {
    res = Call{};
    res.end_bit = start_bit;
    out.clear();
    const uint32_t stride = piece_stride(piece_bytes);
    HostIn in{comp};
    // find
    std::vector<uint64_t> starts{start_bit};
    const uint64_t j0 = first_boundary(start_bit, stride), nb = boundary_count(n_bytes, start_bit, stride);
    for (uint64_t j = j0; j < j0 + nb; ++j) {
        const uint64_t from = j * stride * 8, to = (j + 1) * stride * 8 < n_bytes * 8 ? (j + 1) * stride * 8 : n_bytes * 8;
        for (uint64_t bit = from; bit < to; ++bit)
            if (block_candidate(comp, n_bytes, bit)) { starts.push_back(bit); break; }
    }
    // count
    const uint32_t n_pieces = (uint32_t)starts.size();
    std::vector<Piece> pieces(n_pieces);
    std::vector<Work> work(1);
    pf_inflate::NoSync nosync;
    for (uint32_t p = 0; p < n_pieces; ++p) {
        CountSink cs;
        decode_piece(in, (uint32_t)n_bytes, starts[p], starts.data(), n_pieces, p + 1, NO_BIT, ~0ull, cs, work[0], 0u, 1u, nosync, pieces[p]);
    }
    // chain
    std::vector<uint32_t> live;
    std::vector<uint64_t> place;
    uint64_t total = 0;
    Stats st;
    for (uint32_t p = 0;;) {
        const Piece &r = pieces[p];
        live.push_back(p);
        place.push_back(total);
        total += r.symbols;
        st.blocks_stored += r.stored;
        st.blocks_fixed += r.fixed;
        st.blocks_dynamic += r.dynamic;
        res.end_bit = r.end_bit;
        if (r.link == LINK_CLAUSE) { res.clause = r.clause; res.clause_bit = r.end_bit; break; }
        if (r.link == LINK_FINAL) { res.final = 1; break; }
        if (r.link >= n_pieces) break;   // tail
        p = r.link;
    }
    place.push_back(total);
    st.pieces_found = n_pieces;
    st.pieces_live = live.size();
    st.pieces_dead = n_pieces - live.size();
    if (res.clause) { res.end_bit = start_bit; if (stats) *stats = st; return; }
    // decode
    std::vector<uint16_t> stage(total), ring(RING);
    for (size_t k = 0; k < live.size(); ++k) {
        const Piece &r = pieces[live[k]];
        RingSink<pf_inflate::NoSync> sink(ring.data(), stage.data() + place[k], place[k] + n_window, 0u, 1u, nosync);
        Piece again;
        decode_piece(in, (uint32_t)n_bytes, starts[live[k]], nullptr, 0u, 0u, r.end_bit, r.symbols, sink, work[0], 0u, 1u, nosync, again);
        if (again.link != LINK_LIMIT || again.symbols != r.symbols) {
            res.clause = again.clause ? again.clause : (uint32_t)CLAUSE_PIECE_LIMIT;
            res.clause_bit = again.end_bit;
            res.end_bit = start_bit;
            res.final = 0;
            if (stats) *stats = st;
            return;
        }
    }
    // window: the markers of every piece's last 32 Ki symbols, the pieces in order
    for (size_t k = 0; k < live.size(); ++k) {
        const uint64_t n = place[k + 1] - place[k];
        for (uint64_t s = n > RING ? n - RING : 0; s < n; ++s) {
            uint16_t &v = stage[place[k] + s];
            if (v & MARKER) v = (uint16_t)(RESOLVED | behind(stage.data(), window, n_window, place[k], v));   // (RESOLVED keeps it counted below)
        }
    }
    // resolve: every remaining marker by the same gather
    out.resize(total);
    size_t k = 0;
    for (uint64_t i = 0; i < total; ++i) {
        while (i >= place[k + 1]) ++k;
        const uint16_t v = stage[i];
        if (v & (MARKER | RESOLVED)) ++st.markers;
        out[i] = (uint8_t)((v & MARKER) ? behind(stage.data(), window, n_window, place[k], v) : (v & 0xff));
    }
    if (stats) { st.bytes_out = total; st.bytes_in = (res.end_bit + 7) / 8 - start_bit / 8; *stats = st; }
    res.out_bytes = total;
    res.crc_raw = pf_inflate::crc_raw(out.data(), 0u, (uint32_t)total);
    const uint64_t have = (uint64_t)n_window + total;
    res.n_window = (uint32_t)(have < RING ? have : RING);
    for (uint32_t i = 0; i < res.n_window; ++i) {
        const int64_t q = (int64_t)total - (int64_t)res.n_window + (int64_t)i;
        new_window[i] = q >= 0 ? out[(size_t)q] : window[(int64_t)n_window + q];
    }
}

// ---- one gzip file, block by block: what both streams and gunzip_file below run ----
// call(bytes, n, start_bit, fresh, res, err) inflates bytes[0, n) from start_bit on and puts the text wherever the caller keeps it; it
// keeps the member's window itself and empties it when `fresh` (a member's first call).  false: err is worded (a device error).
struct Stream {
    enum State { HEADER, BODY, TRAILER };
    std::vector<uint8_t> carry;   // the file's bytes behind the last complete block (or header, or trailer)
    uint64_t carry_off = 0;       // where carry[0] lies in the file
    State state = HEADER;
    uint64_t member = 0;          // 0-based
    uint64_t start_bit = 0;       // of the stream within carry[0]
    bool fresh = true;
    uint32_t crc_raw = 0;
    uint64_t len = 0;
    uint64_t carry_max = CARRY_MAX;
    int clause = 0;               // after feed() returned false with an empty err: the refusal
    uint64_t clause_byte = 0;

    void drop(uint64_t n) {
        carry.erase(carry.begin(), carry.begin() + (long)n);
        carry_off += n;
    }
    bool refuse(int c, uint64_t byte) { clause = c; clause_byte = byte; return false; }
    bool done() const { return state == HEADER && carry.empty() && member > 0; }

    template <typename CallFn>
    bool feed(const uint8_t *block, uint64_t n, bool eof, CallFn &&call, std::string &err) {
        if (n) carry.insert(carry.end(), block, block + n);
        for (;;) {
            if (state == HEADER) {
                if (carry.empty() && eof && member > 0) return true;
                uint64_t hl = 0;
                int c = gzip_header(carry.data(), carry.size(), &hl);
                if (c == CLAUSE_HEADER_PAST && !eof) return true;
                if (c == pf_inflate::CLAUSE_MAGIC && member > 0) c = CLAUSE_TRAILING;
                if (c) return refuse(c, carry_off);
                drop(hl);
                state = BODY;
                start_bit = 0;
                fresh = true;
                crc_raw = 0;
                len = 0;
            }
            if (state == BODY) {
                Call r;
                if (!call(carry.data(), (uint64_t)carry.size(), start_bit, fresh, r, err)) return false;
                if (r.clause) return refuse((int)r.clause, carry_off + r.clause_bit / 8);
                fresh = false;
                crc_raw = crc_append(crc_raw, r.crc_raw, r.out_bytes);
                len += r.out_bytes;
                if (r.final) {
                    drop((r.end_bit + 7) / 8);
                    state = TRAILER;
                } else {
                    const bool progress = r.end_bit > start_bit;
                    drop(r.end_bit / 8);
                    start_bit = r.end_bit & 7;
                    if (!progress) {
                        if (eof) return refuse(CLAUSE_CUT_BLOCK, carry_off);
                        if (carry.size() > carry_max) return refuse(CLAUSE_BLOCK_TOO_LARGE, carry_off);
                        return true;
                    }
                    if (!eof) return true;
                    continue;
                }
            }
            if (state == TRAILER) {
                if (carry.size() < 8) return eof ? refuse(CLAUSE_CUT_TRAILER, carry_off) : true;
                const uint8_t *t = carry.data();
                const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
                const uint32_t isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
                if ((uint32_t)len != isize) return refuse(pf_inflate::CLAUSE_LENGTH, carry_off + 4);
                if (pf_inflate::crc_finish(crc_raw, len) != crc) return refuse(pf_inflate::CLAUSE_CRC, carry_off);
                drop(8);
                ++member;
                state = HEADER;
            }
        }
    }
};

// a whole file in memory through Stream and inflate_call, in blocks of block_bytes (0: at once).  Returns the clause (0: text holds the
// members' texts one behind the other); *member (0-based) and *byte say where.
inline int gunzip_file(const uint8_t *bytes, uint64_t n, uint32_t piece_bytes, uint64_t block_bytes, std::vector<uint8_t> &text, uint64_t *member,
                       uint64_t *byte, Stats *stats = nullptr, uint64_t carry_max = CARRY_MAX) {
    Stream s;
    s.carry_max = carry_max;
    std::vector<uint8_t> win[2] = {std::vector<uint8_t>(RING), std::vector<uint8_t>(RING)}, piece_text;
    uint32_t n_window = 0;
    int cur = 0;
    Stats sum;
    text.clear();
    auto call = [&](const uint8_t *p, uint64_t np, uint64_t start_bit, bool fresh, Call &r, std::string &) {
        if (fresh) n_window = 0;
        Stats st;
        inflate_call(p, np, start_bit, win[cur].data(), n_window, piece_bytes, piece_text, win[cur ^ 1].data(), r, &st);
        if (r.clause) return true;
        text.insert(text.end(), piece_text.begin(), piece_text.end());
        n_window = r.n_window;
        cur ^= 1;
        sum.pieces_found += st.pieces_found; sum.pieces_live += st.pieces_live; sum.pieces_dead += st.pieces_dead; sum.markers += st.markers;
        sum.blocks_stored += st.blocks_stored; sum.blocks_fixed += st.blocks_fixed; sum.blocks_dynamic += st.blocks_dynamic;
        sum.bytes_in += st.bytes_in; sum.bytes_out += st.bytes_out;
        return true;
    };
    std::string err;
    const uint64_t step = block_bytes ? block_bytes : (n ? n : 1);
    bool ok = true;
    uint64_t at = 0;
    do {
        const uint64_t take = n - at < step ? n - at : step;
        ok = s.feed(bytes + at, take, at + take >= n, call, err);
        at += take;
    } while (ok && at < n);
    if (member) *member = s.member;
    if (byte) *byte = s.clause_byte;
    if (stats) *stats = sum;
    if (!ok) { text.clear(); return s.clause ? s.clause : (int)CLAUSE_PIECE_LIMIT; }
    return 0;
}

}  // namespace pf_gunzip
