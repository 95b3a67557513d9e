// What both gzip readers' host rules answer on sound and broken deflate streams, one line per input, for comparing two versions of the
// headers byte for byte (plain g++ with -fsanitize=address,undefined; only the rule-level calls inflate_member, inflate_call and
// gunzip_file are used, so the program compiles against any version that has them).
//   gz_decode_dump records.bin budget
// records.bin holds records as tests/cpp/test_gunzip_rule.cpp reads them (u32 tag, u32 length, bytes; repeated):
//   1 a raw deflate stream, 2 its text (behind its 1)
//   4 a deflate stream that is refused; its first byte is the clause (not looked at here)
// Every stream is run as it is and mutated, deterministically: cut at n bytes and with one bit flipped.  A stream of `len` bytes gets
// max(8, budget / len) mutations, half cuts and half flips at evenly spaced places -- every cut and every flip when there are no more
// than that.  Each input goes through
//   m  inflate_member with ISIZE = the text's length (texts of at most 65536 bytes)
//   c  inflate_call at piece strides 64 (streams of at most 2048 bytes) and 2^30
//   f  gunzip_file of a member around it, in blocks of 997 bytes (streams of at most 2048 bytes) or at once
// over heap buffers of exactly the inputs' sizes.  A line: the driver, the clause, the bytes produced, the end bit (and where a clause
// lies), the block counters and a hash of the text.  The last line counts the inputs.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pf_gunzip_rule.hpp"

typedef std::vector<uint8_t> Bytes;

static uint64_t hash_of(const uint8_t *p, size_t n) {   // FNV-1a
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}
static void put32(Bytes &b, uint32_t v) { for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i))); }

struct Record { uint32_t tag; Bytes bytes; };
static std::vector<Record> read_records(const char *path) {
    std::vector<Record> out;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint32_t head[2];
    while (fread(head, 4, 2, f) == 2) {
        Record r;
        r.tag = head[0];
        r.bytes.resize(head[1]);
        if (head[1] && fread(r.bytes.data(), 1, head[1], f) != head[1]) { fprintf(stderr, "short record\n"); exit(2); }
        out.push_back(r);
    }
    fclose(f);
    return out;
}

static void run_member(const Bytes &in, const Bytes &text) {
    if (text.size() > pf_inflate::MAX_ISIZE) return;
    Bytes exact(in.begin(), in.end()), out(text.size());
    int clause = 0;
    pf_inflate::Blocks b = {0, 0, 0};
    uint32_t produced = 0;
    const bool ok = pf_inflate::inflate_member(exact.data(), (uint32_t)exact.size(), out.data(), (uint32_t)out.size(), &clause, &b, &produced);
    printf(" m %d %d %u %u %u %u %016llx\n", (int)ok, clause, produced, b.stored, b.fixed, b.dynamic, (unsigned long long)hash_of(out.data(), produced));
}

static void run_call(const Bytes &in, uint32_t piece) {
    Bytes exact(in.begin(), in.end()), out, new_window(pf_gunzip::RING);
    pf_gunzip::Call r;
    pf_gunzip::Stats st;
    pf_gunzip::inflate_call(exact.data(), exact.size(), 0, nullptr, 0, piece, out, new_window.data(), r, &st);
    printf(" c %u %llu %llu %u %u %08x %llu | %llu %llu %llu %llu %llu %llu %llu %016llx %016llx\n", r.clause, (unsigned long long)r.out_bytes, (unsigned long long)r.end_bit,
           r.final, r.n_window, r.crc_raw, (unsigned long long)r.clause_bit, (unsigned long long)st.pieces_found, (unsigned long long)st.pieces_live,
           (unsigned long long)st.markers, (unsigned long long)st.blocks_stored, (unsigned long long)st.blocks_fixed, (unsigned long long)st.blocks_dynamic,
           (unsigned long long)st.bytes_in, (unsigned long long)hash_of(out.data(), out.size()), (unsigned long long)hash_of(new_window.data(), r.n_window));
}

static void run_file(const Bytes &in, const Bytes &text, uint32_t piece, uint64_t block) {
    Bytes file = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    file.insert(file.end(), in.begin(), in.end());
    put32(file, pf_inflate::crc32(text.data(), text.size()));
    put32(file, (uint32_t)text.size());
    Bytes exact(file.begin(), file.end()), out;
    uint64_t member = 0, byte = 0;
    pf_gunzip::Stats st;
    const int clause = pf_gunzip::gunzip_file(exact.data(), exact.size(), piece, block, out, &member, &byte, &st);
    printf(" f %d %llu %llu %llu | %llu %llu %llu %016llx\n", clause, (unsigned long long)member, (unsigned long long)byte, (unsigned long long)out.size(),
           (unsigned long long)st.blocks_stored, (unsigned long long)st.blocks_fixed, (unsigned long long)st.blocks_dynamic, (unsigned long long)hash_of(out.data(), out.size()));
}

static size_t n_inputs = 0;
static void run_input(const Bytes &in, const Bytes &text, size_t rec, const char *what, size_t where) {
    printf("%zu %s %zu\n", rec, what, where);
    const bool small = in.size() <= 2048;
    run_member(in, text);
    if (small) run_call(in, 64);
    run_call(in, 1u << 30);
    run_file(in, text, small ? 64u : 1u << 30, small ? 997 : 0);
    ++n_inputs;
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: gz_decode_dump records.bin budget\n"); return 2; }
    const std::vector<Record> recs = read_records(argv[1]);
    const size_t budget = (size_t)strtoull(argv[2], nullptr, 10);
    const Bytes none;
    for (size_t i = 0; i < recs.size(); ++i) {
        if (recs[i].tag != 1 && recs[i].tag != 4) continue;
        const Bytes stream = recs[i].tag == 4 ? Bytes(recs[i].bytes.begin() + 1, recs[i].bytes.end()) : recs[i].bytes;
        const Bytes &text = recs[i].tag == 1 && i + 1 < recs.size() && recs[i + 1].tag == 2 ? recs[i + 1].bytes : none;
        run_input(stream, text, i, "whole", 0);
        const size_t len = stream.size(), want = std::max<size_t>(8, len ? budget / len : 0);
        const size_t n_cut = std::min(len, want / 2), n_flip = std::min(8 * len, want - n_cut);
        for (size_t k = 0; k < n_cut; ++k) {
            const size_t n = k * len / n_cut;
            run_input(Bytes(stream.begin(), stream.begin() + (long)n), text, i, "cut", n);
        }
        for (size_t k = 0; k < n_flip; ++k) {
            const size_t bit = k * (8 * len) / n_flip;
            Bytes bad = stream;
            bad[bit / 8] ^= (uint8_t)(1u << (bit % 8));
            run_input(bad, text, i, "flip", bit);
        }
    }
    printf("inputs %zu\n", n_inputs);
    return 0;
}
