// The rule of K-INFLATE (blocked gzip, `--gz`) in one place, for the host layer (host/pf_reads_stream.cpp, host/pf_gz_host.cpp), the
// kernel's error texts (pf_inflate.hip) and the stand-alone test (tests/cpp/test_inflate_rule.cpp).
//
// Blocked gzip (BGZF, what `bgzip`, bcl2fastq2 and BCL Convert write) is a sequence of gzip members (RFC 1952), each
//   1f 8b | CM = 8 | FLG = 4 (FEXTRA) | MTIME XFL OS (6 bytes, not looked at) | XLEN | subfields, among them 'B' 'C' 02 00 BSIZE |
//   a deflate stream (RFC 1951) | CRC32 | ISIZE
// of BSIZE + 1 bytes in all, ISIZE <= 65536, no member referring to another.  The 28-byte end-of-file marker is a member with
// ISIZE = 0.  A gzip file without the BC subfield is one deflate stream whose blocks start at unknown bits and reach 32 KiB back: it
// is refused by name (CLAUSE_NOT_BLOCKED), as is everything else a member can get wrong, one clause each.
//
// The decoder itself is pf_inflate_core.hpp, the same code the kernel runs per lane; here it runs as lane 0 of 1 over plain memory.
#pragma once
#include <stdint.h>
#include <string.h>

#include "pf_inflate_core.hpp"

namespace pf_inflate {

inline const char *clause_text(int c) {
    switch (c) {
        case CLAUSE_MAGIC: return "the member does not start with the gzip magic 1f 8b";
        case CLAUSE_NOT_BLOCKED:
            return "the input is gzip but not blocked gzip (no BC subfield): one deflate stream cannot be cut for the device; recompress it "
                   "with bgzip, or decompress it";
        case CLAUSE_METHOD: return "the compression method is not 8 (deflate)";
        case CLAUSE_FLAGS: return "the gzip flags are not FEXTRA alone (04) as blocked gzip sets them: recompress the input with bgzip, or decompress it";
        case CLAUSE_SHORT: return "the member is shorter than its header and trailer";
        case CLAUSE_PAST_END: return "the member runs past the end of the file";
        case CLAUSE_ISIZE: return "the member's ISIZE is above 65536";
        case CLAUSE_BTYPE3: return "a deflate block of type 3";
        case CLAUSE_STORED_LEN: return "a stored block whose LEN and NLEN do not match";
        case CLAUSE_STORED_PAST: return "a stored block runs past the payload";
        case CLAUSE_TOO_MANY_CODES: return "more than 286 literal/length or 30 distance codes";
        case CLAUSE_CODE_LENGTHS: return "over-subscribed or incomplete code lengths";
        case CLAUSE_REPEAT: return "a repeat code with nothing to repeat or running past HLIT + HDIST";
        case CLAUSE_NO_EOB: return "a block without an end-of-block code";
        case CLAUSE_BAD_CODE: return "bits that are no code of the block's code lengths";
        case CLAUSE_LITLEN_SYM: return "literal/length symbol 286 or 287";
        case CLAUSE_DIST_SYM: return "distance symbol 30 or 31";
        case CLAUSE_DIST_BEFORE: return "a distance reaches before the member's first byte";
        case CLAUSE_OUT_BEYOND: return "the stream gives more bytes than ISIZE";
        case CLAUSE_END: return "the final block does not end at the trailer";
        case CLAUSE_LENGTH: return "the inflated length differs from ISIZE";
        case CLAUSE_CRC: return "CRC-32 mismatch";
        default: return "no refusal";
    }
}

// ---- container ----
inline int parse_member(const uint8_t *bytes, uint64_t n, Header *hdr) {
    Header h;
    const int c = parse_member_bytes(bytes, n, h);
    if (hdr) *hdr = h;
    return c;
}

// What the first bytes of a file say with `--gz` (first[0, n_first) of a file of file_size bytes; 65536 bytes hold any first member).
// FILE_PLAIN: no gzip magic, read as it is today (FASTA and the rest are pf_mask::file_clause's); FILE_BGZF; or FILE_REFUSED with *clause.
enum FileKind { FILE_PLAIN = 0, FILE_BGZF = 1, FILE_REFUSED = 2 };
inline int file_clause_gz(const uint8_t *first, uint64_t n_first, uint64_t file_size, int *clause) {
    if (clause) *clause = CLAUSE_NONE;
    if (n_first < 2 || first[0] != 0x1f || first[1] != 0x8b) return FILE_PLAIN;
    Header h;
    int c = parse_member_bytes(first, n_first, h);
    // (a header cut by the n_first bytes looked at, not by the file, cannot be judged further: members are at most 65536 bytes)
    if (c == CLAUSE_PAST_END && n_first < file_size && n_first >= 65536) c = CLAUSE_NONE;
    if (c == CLAUSE_ISIZE) c = CLAUSE_NONE;   // (a member clause: refused once the stream runs, with its number and offset)
    if (clause) *clause = c;
    return c ? FILE_REFUSED : FILE_BGZF;
}

// ---- stream: the core over plain memory ----
struct HostIn {   // (for pf_gunzip_rule.hpp as well)
    const uint8_t *p;
    uint8_t byte(uint32_t i) const { return p[i]; }
    uint8_t raw(uint32_t i) const { return p[i]; }
};
struct HostOut {   // a member's text: nothing in front of it, places of 32 bits
    typedef uint32_t Pos;
    static constexpr int BEYOND = CLAUSE_OUT_BEYOND;
    uint8_t *p;
    uint32_t reach() const { return 0; }
    void put(uint32_t at, uint8_t b) { p[at] = b; }
    void copy(uint32_t at, uint32_t dist, uint32_t len) {   // dist < len: the pattern repeats
        for (uint32_t i = 0; i < len; ++i) p[at + i] = p[at - dist + (i % dist)];
    }
    void stored(const HostIn &in, uint32_t src, uint32_t at, uint32_t len) {
        for (uint32_t i = 0; i < len; ++i) p[at + i] = in.raw(src + i);
    }
};

inline uint32_t crc32(const uint8_t *bytes, uint64_t n) {
    uint32_t reg = 0xffffffffu;
    for (uint64_t i = 0; i < n; ++i) reg = crc_byte(reg, bytes[i]);
    return ~reg;
}
// the same from n_lanes slices, as the kernel's lanes compute it
inline uint32_t crc32_sliced(const uint8_t *bytes, uint32_t n, uint32_t n_lanes) {
    uint32_t sum = 0;
    for (uint32_t j = 0; j < n_lanes; ++j)
        sum ^= slice_share(crc_raw(bytes, slice_begin(n, n_lanes, j), slice_end(n, n_lanes, j)), n, n_lanes, j);
    return crc_finish(sum, n);
}

// payload[0, n_in) -> out[0, isize): true when the stream is sound and gives exactly isize bytes (the CRC is the caller's: the trailer
// is not part of the payload).  Reads nothing outside the payload and writes nothing outside out[0, isize), whatever the bytes say.
inline bool inflate_member(const uint8_t *payload, uint32_t n_in, uint8_t *out, uint32_t isize, int *clause, Blocks *blocks = nullptr,
                           uint32_t *produced = nullptr) {
    Work w;
    HostIn in{payload};
    HostOut o{out};
    Blocks b;
    uint32_t made = 0;
    const int c = inflate_stream(in, n_in, o, isize, w, 0u, 1u, NoSync{}, b, made);
    if (clause) *clause = c;
    if (blocks) *blocks = b;
    if (produced) *produced = made;
    return c == CLAUSE_NONE;
}

// a whole member at bytes[0, n): header, stream, length, CRC.  out holds 65536 bytes.  Returns the clause; *out_len = ISIZE.
inline int inflate_bgzf_member(const uint8_t *bytes, uint64_t n, uint8_t *out, uint32_t *out_len, Blocks *blocks = nullptr) {
    if (out_len) *out_len = 0;
    Header h;
    int c = parse_member_bytes(bytes, n, h);
    if (c) return c;
    if (!inflate_member(bytes + h.payload_off, h.member_len - h.payload_off - TRAILER, out, h.isize, &c, blocks)) return c;
    if (crc32_sliced(out, h.isize, 64) != h.crc) return CLAUSE_CRC;
    if (out_len) *out_len = h.isize;
    return CLAUSE_NONE;
}

}  // namespace pf_inflate
