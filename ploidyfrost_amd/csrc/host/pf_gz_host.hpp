// The inputs of the reads sub-commands, block by block, and the device side of the compressed ones (`--gz`, `--gz-plain`): what the
// two streams of pf_reads_stream.hpp share.
//   BlockReader  the reader thread's side, one per open file, by the file's kind.  Text and plain gzip: the next bytes as they are.
//                Blocked gzip: hops from member header to member header by BSIZE (no decoding on the host) and packs whole members
//                into the buffer with their offset table, until the next member's ISIZE would take the inflated sum past the chunk,
//                or its bytes past the buffer.  Such a block always holds at least one member.
//   GzText       the device loop's side: the compressed block is uploaded, K-INFLATE (pf_inflate_bgzf) writes its text behind what is
//                left of the text before it, and the step gets a device pointer.  The carry -- the bytes behind the last whole record
//                -- stays on the device: it is copied device to device to the front of the other of two text buffers.  The inflated
//                text never crosses PCIe (a trim log, which is written on the host, fetches it).
// The rule, the refusals and their texts are ../pf_inflate_rule.hpp.
//
// Plain gzip (`--gz-plain`, any gzip that is not blocked): the reader hands over raw blocks of gz_plain_block(chunk) bytes and decodes
// nothing; GzText::append_plain runs pf_gunzip::Stream (../pf_gunzip_rule.hpp) over them -- the container on the host, a host carry of
// the compressed bytes behind the last complete deflate block, K-GUNZIP (pf_inflate_gzip) on carry + block with the member's window
// kept on the device -- and the text goes behind the carried record end exactly as above.
#pragma once
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "ploidyfrost_hip.h"

namespace pfh {

constexpr uint64_t GZ_MEMBER_MAX = 1u << 16;   // bytes of a member, compressed or inflated

// what an input is, by its first bytes (the preflight of pf_reads_stream.hpp decides it, once): text as it is, blocked gzip for
// K-INFLATE, or any other gzip for K-GUNZIP
enum GzKind { GZ_KIND_TEXT = 0, GZ_KIND_BGZF = 1, GZ_KIND_GZIP = 3 };
// bytes of a plain-gzip file the reader hands over at a time
inline uint64_t gz_plain_block(uint64_t chunk) { return chunk / 4 > (64u << 10) ? chunk / 4 : (64u << 10); }
// bytes of pinned buffer a reader of chunks of `chunk` inflated bytes fills: empty members make compressed exceed inflated
inline uint64_t gz_buffer_bytes(uint64_t chunk) { return (chunk > GZ_MEMBER_MAX ? chunk : GZ_MEMBER_MAX) + 2 * GZ_MEMBER_MAX; }

struct FileBlock {
    uint64_t len = 0;            // bytes of the file (blocked gzip: whole members)
    uint64_t file_off = 0;       // where they start in the file
    bool eof = false;            // the file ends with them
    // blocked gzip alone
    uint64_t inflated = 0;       // the sum of the members' ISIZE
    uint64_t first_member = 0;   // the 0-based number of the first in the file
    std::vector<uint64_t> member_off;   // members + 1 offsets into the block
};

struct BlockReader {
    int fd = -1;
    GzKind kind = GZ_KIND_TEXT;
    std::string who, path;
    uint64_t pos = 0, members = 0;
    std::vector<char> ahead;   // blocked gzip: bytes read behind the last member handed over: the next block starts with them, nothing is read twice
    bool open_file(const std::string &who_, const std::string &path_, GzKind kind_, std::string &err);
    void close_file();
    // bytes of buffer a block of a file of this kind takes at most, for chunks of `chunk` bytes of text
    static uint64_t block_bytes(GzKind kind, uint64_t chunk) {
        return kind == GZ_KIND_BGZF ? gz_buffer_bytes(chunk) : kind == GZ_KIND_GZIP ? gz_plain_block(chunk) : chunk;
    }
    // the next block into buf[0, cap): min(cap, block_bytes(kind, chunk)) bytes as they are, or (blocked gzip, cap >=
    // gz_buffer_bytes(chunk)) whole members.  false: err is worded (the read error, or `who: path: member N, byte B: clause`)
    bool next(char *buf, uint64_t cap, uint64_t chunk, FileBlock &b, std::string &err);
    ~BlockReader() { close_file(); }

private:
    bool next_members(char *buf, uint64_t cap, uint64_t chunk, FileBlock &b, std::string &err);
};

struct GzText {
    pf_ctx *ctx = nullptr;
    char *d_comp = nullptr, *d_text[2] = {nullptr, nullptr};
    uint64_t *d_off = nullptr;
    uint64_t comp_cap = 0, off_cap = 0, text_cap[2] = {0, 0};
    int cur = 0;
    uint64_t begin = 0, end = 0;   // the text not yet used: d_text[cur][begin, end)
    explicit GzText(pf_ctx *c);
    GzText(const GzText &) = delete;
    GzText &operator=(const GzText &) = delete;
    ~GzText();
    const char *text() const { return d_text[cur] ? d_text[cur] + begin : nullptr; }
    uint64_t size() const { return end - begin; }
    void use(uint64_t bytes) { begin += bytes; }
    // what is left moves to the front of the other buffer and the block's text goes behind it.  false: err is worded
    bool append(const std::string &who, const std::string &path, const char *comp, const FileBlock &b, std::string &err);
    bool fetch(std::vector<char> &host, std::string &err) const;   // the text not yet used, to the host
    // plain gzip: `len` raw bytes of the file from file offset file_off on (0: a new file), eof = its last.  false: err is worded
    bool append_plain(const std::string &who, const std::string &path, const char *raw, uint64_t len, uint64_t file_off, bool eof, std::string &err);

private:
    struct Plain;                  // the gzip file's state: pf_gunzip::Stream, the window on the device
    std::unique_ptr<Plain> plain;
};

}  // namespace pfh
