// Blocked-gzip inputs of the reads sub-commands (`--gz`): what the two stream seams (stream_fastq_sized in pf_mask_host.cpp,
// stream_fastq_pair in pf_trim_host.cpp) share.
//   GzReader   the reader thread's side: hops from member header to member header by BSIZE (no decoding on the host) and packs whole
//              members into a pinned buffer with their offset table, until the next member's ISIZE would take the inflated sum past
//              the chunk, or its bytes past the buffer.  A block always holds at least one member.
//   GzText     the device loop's side: the compressed block is uploaded, K-INFLATE (pf_inflate_bgzf) writes its text behind what is
//              left of the text before it, and the step gets a device pointer.  The carry -- the bytes behind the last whole record
//              -- stays on the device: it is copied device to device to the front of the other of two text buffers.  The inflated
//              text never crosses PCIe (a trim log, which is written on the host, fetches it).
// The rule, the refusals and their texts are ../pf_inflate_rule.hpp.
//
// Plain gzip (`--gz-plain`, any gzip that is not blocked): the reader thread reads raw blocks of gz_plain_block(chunk) bytes and decodes
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

// what an input is under the switch gz (0 none, 1 `--gz`, 2 `--gz-plain`), by its first bytes: text as it is, blocked gzip for
// K-INFLATE, or (2 only) any other gzip for K-GUNZIP.  The preflight has refused what is refused.
enum GzKind { GZ_KIND_TEXT = 0, GZ_KIND_BGZF = 1, GZ_KIND_GZIP = 3 };
int gz_kind(const std::string &path, int gz);
// bytes of a plain-gzip file the reader hands over at a time
inline uint64_t gz_plain_block(uint64_t chunk) { return chunk / 4 > (64u << 10) ? chunk / 4 : (64u << 10); }

// does the file start with the gzip magic?  (false when it cannot be read: the caller's open() words that)
bool gz_magic(const std::string &path);
// bytes of pinned buffer a reader of chunks of `chunk` inflated bytes fills: empty members make compressed exceed inflated
inline uint64_t gz_buffer_bytes(uint64_t chunk) { return (chunk > GZ_MEMBER_MAX ? chunk : GZ_MEMBER_MAX) + 2 * GZ_MEMBER_MAX; }

struct GzBlock {
    uint64_t len = 0;            // compressed bytes, whole members
    uint64_t inflated = 0;       // the sum of their ISIZE
    uint64_t file_off = 0;       // where the first of them starts in the file
    uint64_t first_member = 0;   // its 0-based number in the file
    std::vector<uint64_t> member_off;   // members + 1 offsets into the block
    bool eof = false;
    bool plain = false;          // raw bytes of a plain-gzip file: only len, file_off and eof are set
};

struct GzReader {
    int fd = -1;
    std::string who, path;
    uint64_t pos = 0, members = 0;
    std::vector<char> ahead;   // bytes read behind the last member handed over: the next block starts with them, nothing is read twice
    bool open_file(const std::string &who_, const std::string &path_, std::string &err);
    void close_file();
    // the next block into buf[0, cap), cap >= gz_buffer_bytes(chunk).  false: err is worded (`who: path: member N, byte B: clause`, or
    // the read error)
    bool next(char *buf, uint64_t cap, uint64_t chunk, GzBlock &b, std::string &err);
    // the same for a plain-gzip file: the next `want` <= cap bytes as they are
    bool next_raw(char *buf, uint64_t want, GzBlock &b, std::string &err);
    ~GzReader() { close_file(); }
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
    bool append(const std::string &who, const std::string &path, const char *comp, const GzBlock &b, std::string &err);
    bool fetch(std::vector<char> &host, std::string &err) const;   // the text not yet used, to the host
    // plain gzip: `len` raw bytes of the file from file offset file_off on (0: a new file), eof = its last.  false: err is worded
    bool append_plain(const std::string &who, const std::string &path, const char *raw, uint64_t len, uint64_t file_off, bool eof, std::string &err);

private:
    struct Plain;                  // the gzip file's state: pf_gunzip::Stream, the window on the device
    std::unique_ptr<Plain> plain;
};

}  // namespace pfh
