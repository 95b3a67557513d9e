// The rule of K-GUNZIP alone (pf_gunzip_rule.hpp over pf_gunzip_core.hpp and pf_inflate_core.hpp), for plain g++ with
// -fsanitize=address,undefined: the container and its clauses on files written here (stored blocks), a file cut at every byte, the
// carry bound, and -- with a file name -- the records the Python test makes with zlib (u32 tag, u32 length, bytes; repeated):
//   1 a gzip file, 2 its text: inflated for several piece strides and block sizes, and cut at every byte
//   3 a gzip file of about 300 bytes, 2 its text: every single bit flipped in turn; the answer is the right text or a clause
//   4 a deflate stream that is refused; its first byte is the clause
//   5 a deflate stream that starts with a non-final dynamic block and ends at a byte boundary: planted in a stored block's bytes as a
//     false candidate, which the chain must pass over
// Everything runs over heap buffers of exactly the inputs' sizes, so that a read or write outside them stops the program.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pf_gunzip_rule.hpp"

using namespace pf_gunzip;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED line %d: %s\n", __LINE__, #c);               \
            exit(1);                                                    \
        }                                                               \
    } while (0)

typedef std::vector<uint8_t> Bytes;

static void put32(Bytes &b, uint32_t v) { for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i))); }
static Bytes text_of(size_t n, uint32_t seed) {
    Bytes t(n);
    for (size_t i = 0; i < n; ++i) { seed = seed * 1664525u + 1013904223u; t[i] = (uint8_t)"ACGTN@+\nI"[(seed >> 24) % 9]; }
    return t;
}
// stored blocks of at most `block` bytes; the last one final
static Bytes stored_stream(const Bytes &text, size_t block, bool final = true) {
    Bytes s;
    size_t at = 0;
    do {
        const size_t n = text.size() - at < block ? text.size() - at : block;
        s.push_back((uint8_t)((final && at + n == text.size()) ? 1 : 0));
        s.push_back((uint8_t)n); s.push_back((uint8_t)(n >> 8)); s.push_back((uint8_t)~n); s.push_back((uint8_t)(~n >> 8));
        s.insert(s.end(), text.begin() + (long)at, text.begin() + (long)(at + n));
        at += n;
    } while (at < text.size());
    return s;
}
static Bytes header(uint8_t flg) {
    Bytes h = {0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 3};
    if (flg & 4) { h.push_back(5); h.push_back(0); for (int i = 0; i < 5; ++i) h.push_back((uint8_t)('a' + i)); }
    if (flg & 8) { for (const char *c = "name.fq"; *c; ++c) h.push_back((uint8_t)*c); h.push_back(0); }
    if (flg & 16) { for (const char *c = "a comment"; *c; ++c) h.push_back((uint8_t)*c); h.push_back(0); }
    if (flg & 2) { h.push_back(0x12); h.push_back(0x34); }
    return h;
}
static Bytes member(const Bytes &text, const Bytes &stream, uint8_t flg = 0) {
    Bytes m = header(flg);
    m.insert(m.end(), stream.begin(), stream.end());
    put32(m, pf_inflate::crc32(text.data(), text.size()));
    put32(m, (uint32_t)text.size());
    return m;
}
static Bytes cat(const Bytes &a, const Bytes &b) { Bytes c = a; c.insert(c.end(), b.begin(), b.end()); return c; }

struct Answer { int clause; uint64_t member, byte; Bytes text; Stats st; };
static Answer run_file(const Bytes &file, uint32_t piece, uint64_t block, uint64_t carry_max = CARRY_MAX) {
    Bytes exact(file);   // (its own allocation of exactly the file's size)
    exact.shrink_to_fit();
    Answer a;
    a.clause = gunzip_file(exact.data(), exact.size(), piece, block, a.text, &a.member, &a.byte, &a.st, carry_max);
    return a;
}

static void container() {
    for (int flg = 0; flg < 32; ++flg) {
        const Bytes h = header((uint8_t)flg);
        uint64_t len = 0;
        for (size_t n = 0; n < h.size(); ++n) {
            Bytes cut(h.begin(), h.begin() + (long)n);
            cut.shrink_to_fit();
            CHECK(gzip_header(cut.data(), cut.size(), &len) == CLAUSE_HEADER_PAST);
        }
        CHECK(gzip_header(h.data(), h.size(), &len) == 0 && len == h.size());
    }
    uint64_t len = 0;
    Bytes h = header(0);
    h[2] = 7;
    CHECK(gzip_header(h.data(), h.size(), &len) == pf_inflate::CLAUSE_METHOD);
    for (int bit = 5; bit < 8; ++bit) { h = header(0); h[3] = (uint8_t)(1 << bit); CHECK(gzip_header(h.data(), h.size(), &len) == CLAUSE_RESERVED_FLAG); }
    h = header(0);
    h[1] = 0x8c;
    CHECK(gzip_header(h.data(), h.size(), &len) == pf_inflate::CLAUSE_MAGIC);
    for (int c = 1; c < CLAUSE_END_; ++c) CHECK(strcmp(clause_text(c), "no refusal") != 0);
    int clause = 0;
    h = header(8);
    CHECK(file_kind(h.data(), h.size(), 1000, &clause) == FILE_GZIP && clause == 0);
    CHECK(file_kind(h.data(), 12, 12, &clause) == FILE_REFUSED && clause == CLAUSE_HEADER_PAST);
    CHECK(file_kind((const uint8_t *)"@r\n", 3, 3, &clause) == FILE_PLAIN);
    h = header(4);   // FLG = 04 without a BC subfield: not blocked, so plain gzip
    CHECK(file_kind(h.data(), h.size(), 1000, &clause) == FILE_GZIP);
    const uint8_t bgzf_eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(file_kind(bgzf_eof, 28, 28, &clause) == FILE_BGZF);
}

static void files_of_stored_blocks() {
    const Bytes a = text_of(1000, 1), b = text_of(77, 2), none;
    const Bytes file = cat(cat(member(a, stored_stream(a, 300), 8), member(none, stored_stream(none, 10))), member(b, stored_stream(b, 1000), 2 | 4 | 16));
    const Bytes want = cat(a, b);
    for (uint32_t piece : {64u, 1024u})
        for (uint64_t block : {(uint64_t)0, (uint64_t)1, (uint64_t)7, (uint64_t)64, (uint64_t)500}) {
            const Answer r = run_file(file, piece, block);
            CHECK(r.clause == 0 && r.text == want && r.member == 3 && r.st.blocks_stored == 6 && r.st.pieces_dead == 0);
        }
    // cut at every byte: a clause that says where the file ends, never the whole text
    for (size_t n = 0; n < file.size(); ++n) {
        const Answer r = run_file(Bytes(file.begin(), file.begin() + (long)n), 64, n % 3 ? 50 : 0);
        const size_t m1 = member(a, stored_stream(a, 300), 8).size(), m2 = m1 + member(none, stored_stream(none, 10)).size();
        if (n == m1 || n == m2) { CHECK(r.clause == 0); continue; }   // (whole members: a sound, shorter file)
        CHECK(r.clause == CLAUSE_HEADER_PAST || r.clause == CLAUSE_CUT_BLOCK || r.clause == CLAUSE_CUT_TRAILER);
        CHECK(r.text.empty() && r.byte <= n && r.member == (n < m1 ? 0u : n < m2 ? 1u : 2u));
    }
    // the trailer and what follows it
    Bytes bad = file;
    bad[bad.size() - 1] ^= 1;
    Answer r = run_file(bad, 64, 0);
    CHECK(r.clause == pf_inflate::CLAUSE_LENGTH && r.member == 2 && r.byte == file.size() - 4);
    bad = file;
    bad[bad.size() - 7] ^= 0x40;
    r = run_file(bad, 64, 10);
    CHECK(r.clause == pf_inflate::CLAUSE_CRC && r.member == 2 && r.byte == file.size() - 8);
    bad = cat(file, Bytes{'\n'});
    r = run_file(bad, 64, 0);
    CHECK(r.clause == CLAUSE_TRAILING && r.member == 3 && r.byte == file.size());
    bad = cat(file, Bytes{0x1f, 0x8b, 9});
    r = run_file(bad, 64, 0);
    CHECK(r.clause == pf_inflate::CLAUSE_METHOD && r.member == 3 && r.byte == file.size());
    bad = file;
    bad[header(8).size() + 3] ^= 0x80;   // NLEN of the first stored block
    r = run_file(bad, 64, 0);
    CHECK(r.clause == pf_inflate::CLAUSE_STORED_LEN && r.member == 0 && r.byte == header(8).size());
    bad = file;
    bad[header(8).size()] = 6;           // BTYPE 3
    r = run_file(bad, 64, 33);
    CHECK(r.clause == pf_inflate::CLAUSE_BTYPE3 && r.member == 0 && r.byte == header(8).size());
    // a block of more compressed bytes than the carry may hold
    r = run_file(file, 64, 16, 128);
    CHECK(r.clause == CLAUSE_BLOCK_TOO_LARGE && r.member == 0 && r.byte == header(8).size());
    r = run_file(file, 64, 16, 400);   // (the largest block is 305 bytes)
    CHECK(r.clause == 0 && r.text == want);
}

struct Record { uint32_t tag; Bytes bytes; };
static std::vector<Record> read_records(const char *path) {
    std::vector<Record> out;
    FILE *f = fopen(path, "rb");
    CHECK(f);
    uint32_t head[2];
    while (fread(head, 4, 2, f) == 2) {
        Record r;
        r.tag = head[0];
        r.bytes.resize(head[1]);
        CHECK(head[1] == 0 || fread(r.bytes.data(), 1, head[1], f) == head[1]);
        out.push_back(r);
    }
    fclose(f);
    return out;
}

static void one_call(const Bytes &stream, uint32_t piece, Call &res, Bytes &out, Stats &st, const Bytes &window = Bytes()) {
    Bytes exact(stream), win(window);
    exact.shrink_to_fit();
    win.shrink_to_fit();
    Bytes new_window(RING);
    inflate_call(exact.data(), exact.size(), 0, win.data(), (uint32_t)win.size(), piece, out, new_window.data(), res, &st);
}

int main(int argc, char **argv) {
    container();
    files_of_stored_blocks();
    if (argc < 2) { printf("ok\n"); return 0; }
    const std::vector<Record> recs = read_records(argv[1]);
    size_t n_files = 0, n_flip = 0, n_refused = 0, n_planted = 0;
    for (size_t i = 0; i < recs.size(); ++i) {
        const Bytes &b = recs[i].bytes;
        if (recs[i].tag == 1) {
            CHECK(i + 1 < recs.size() && recs[i + 1].tag == 2);
            const Bytes &text = recs[i + 1].bytes;
            for (uint32_t piece : {64u, 1024u, 16384u, 1u << 30})
                for (uint64_t block : {(uint64_t)0, (uint64_t)4096, (uint64_t)100}) {
                    const Answer r = run_file(b, piece, block);
                    CHECK(r.clause == 0 && r.text == text);
                }
            for (size_t n = 0; n < b.size(); ++n) {
                const Answer r = run_file(Bytes(b.begin(), b.begin() + (long)n), 64, 0);
                CHECK(r.clause != 0 && r.text.empty() && r.byte <= n);
            }
            ++n_files;
        } else if (recs[i].tag == 3) {
            CHECK(i + 1 < recs.size() && recs[i + 1].tag == 2);
            const Bytes &text = recs[i + 1].bytes;
            size_t refused = 0;
            for (size_t bit = 0; bit < 8 * b.size(); ++bit) {
                Bytes bad = b;
                bad[bit / 8] ^= (uint8_t)(1u << (bit % 8));
                const Answer r = run_file(bad, 64, bit % 2 ? 0 : 50);
                CHECK(r.clause != 0 ? r.text.empty() : r.text == text);   // (a flip of MTIME, XFL, OS or the name changes nothing)
                refused += r.clause != 0;
            }
            CHECK(refused > 8 * b.size() * 3 / 4);
            ++n_flip;
        } else if (recs[i].tag == 4) {
            Call res;
            Bytes out;
            Stats st;
            one_call(Bytes(b.begin() + 1, b.end()), 64, res, out, st);
            CHECK(res.clause == b[0] && res.clause_bit == 0 && out.empty() && res.end_bit == 0);
            ++n_refused;
        } else if (recs[i].tag == 5) {
            CHECK(block_candidate(b.data(), b.size(), 0));
            Bytes payload = text_of(70, 3);   // the candidate lies behind the first nominal boundary of 64 bytes
            payload.insert(payload.end(), b.begin(), b.end());
            Bytes stream = stored_stream(payload, 65535, false);
            stream.push_back(0x03);   // a final fixed block of no symbols
            stream.push_back(0x00);
            CHECK(block_candidate(stream.data(), stream.size(), 8 * 75));
            Call res;
            Bytes out;
            Stats st;
            one_call(stream, 64, res, out, st);
            CHECK(res.clause == 0 && res.final == 1 && out == payload);
            CHECK(st.pieces_found >= 2 && st.pieces_live == 1 && st.pieces_dead == st.pieces_found - 1 && st.blocks_stored == 1 && st.blocks_dynamic == 0);
            ++n_planted;
        }
    }
    CHECK(n_files >= 1 && n_flip >= 1 && n_refused >= 9 && n_planted >= 1);
    printf("ok\n");
    return 0;
}
