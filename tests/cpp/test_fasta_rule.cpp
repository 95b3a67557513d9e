// Stand-alone test of csrc/pf_fasta_rule.hpp (the header alone, no device, no library): built with plain g++ and
// -fsanitize=address,undefined by tests/test_fasta_cpu.py.  Every text lives in a heap buffer of exactly its size, so that a read
// one byte past a chunk is caught.  Checked: the hand-made texts against expected sequences; the word form (the stages of the kernel,
// index_fasta_words) against the line form (index_fasta) on every text, final and cut at every byte; and that a text cut at any byte
// as a chunk that is not final, followed by the rest from bytes_used on as the final chunk, gives the records of the whole.
// With an argument: a file of texts, each behind its length as 4 bytes little endian (the edge texts of tests/fasta_cases.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "pf_fasta_rule.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            fprintf(stderr, "line %d: %s: ", __LINE__, #cond);             \
            fprintf(stderr, __VA_ARGS__);                                  \
            fprintf(stderr, "\n");                                         \
        }                                                                  \
    } while (0)

struct Exact {   // n bytes on the heap, not one more
    std::unique_ptr<char[]> p;
    uint64_t n;
    Exact(const char *src, uint64_t len) : p(new char[len ? len : 1]), n(len) { if (len) memcpy(p.get(), src, len); }
};

static std::vector<std::string> reads_of(const pf_fasta::Index &ix) {
    std::vector<std::string> r;
    for (uint64_t i = 0; i < ix.n_records; ++i) r.emplace_back(ix.text.data() + ix.read_off[i], ix.read_len[i]);
    return r;
}
static bool same(const pf_fasta::Index &a, const pf_fasta::Index &b) {
    return a.bytes_used == b.bytes_used && a.n_records == b.n_records && a.bases == b.bases && a.text == b.text && a.read_off == b.read_off &&
           a.read_len == b.read_len;
}

// both forms on text[0, n) in an exact buffer; returns the line form's index
static pf_fasta::Index both(const std::string &name, const char *text, uint64_t n, bool final) {
    const Exact e(text, n);
    pf_fasta::Index a, b;
    const int ca = pf_fasta::index_fasta(e.p.get(), n, final, a), cb = pf_fasta::index_fasta_words(e.p.get(), n, final, b);
    CHECK(ca == cb, "%s: clauses %d and %d at n = %llu final = %d", name.c_str(), ca, cb, (unsigned long long)n, (int)final);
    CHECK(same(a, b), "%s: the word form differs at n = %llu final = %d (records %llu / %llu, bases %llu / %llu, used %llu / %llu)", name.c_str(),
          (unsigned long long)n, (int)final, (unsigned long long)a.n_records, (unsigned long long)b.n_records, (unsigned long long)a.bases,
          (unsigned long long)b.bases, (unsigned long long)a.bytes_used, (unsigned long long)b.bytes_used);
    uint64_t sum = 0;
    for (uint64_t i = 0; i < a.n_records; ++i) {
        CHECK(a.read_off[i] == sum, "%s: the table is not the running sum at record %llu", name.c_str(), (unsigned long long)i);
        sum += a.read_len[i];
    }
    CHECK(sum == a.bases && a.text.size() == a.bases, "%s: bases", name.c_str());
    return a;
}

static void every_cut(const std::string &name, const std::string &text) {
    const pf_fasta::Index whole = both(name, text.data(), text.size(), true);
    CHECK(whole.bytes_used == text.size(), "%s: a final chunk is used up", name.c_str());
    const std::vector<std::string> want = reads_of(whole);
    // (every byte of a text of up to 3000 bytes; of a longer one every byte near its ends and near every multiple of 4096, the
    // compaction kernel's tile, and every 61st in between: the forms are quadratic in the length under the sanitizers)
    for (uint64_t c = 1; c <= text.size(); ++c) {
        const uint64_t m = c % 4096;
        if (text.size() > 3000 && c > 200 && c + 200 < text.size() && m > 70 && m < 4096 - 70 && c % 61) continue;
        const pf_fasta::Index head = both(name, text.data(), c, false);
        CHECK(head.bytes_used <= c, "%s: cut %llu", name.c_str(), (unsigned long long)c);
        CHECK(head.bytes_used == 0 || (text[head.bytes_used] == '>' && text[head.bytes_used - 1] == '\n'), "%s: cut %llu: bytes_used is no header start",
              name.c_str(), (unsigned long long)c);
        CHECK((head.n_records == 0) == (head.bytes_used == 0), "%s: cut %llu: no record, nothing used", name.c_str(), (unsigned long long)c);
        const pf_fasta::Index rest = both(name, text.data() + head.bytes_used, text.size() - head.bytes_used, true);
        std::vector<std::string> got = reads_of(head);
        for (const std::string &r : reads_of(rest)) got.push_back(r);
        CHECK(got == want, "%s: cut %llu: %zu + %llu records, the whole has %zu", name.c_str(), (unsigned long long)c, got.size() - (size_t)rest.n_records,
              (unsigned long long)rest.n_records, want.size());
        CHECK(head.bases + rest.bases == whole.bases, "%s: cut %llu: bases", name.c_str(), (unsigned long long)c);
    }
}

static void expect(const std::string &text, bool final, const std::vector<std::string> &want, uint64_t used) {
    const pf_fasta::Index ix = both(text, text.data(), text.size(), final);
    CHECK(reads_of(ix) == want, "%s (final = %d): %llu records", text.c_str(), (int)final, (unsigned long long)ix.n_records);
    CHECK(ix.bytes_used == used, "%s (final = %d): bytes_used %llu, not %llu", text.c_str(), (int)final, (unsigned long long)ix.bytes_used,
          (unsigned long long)used);
}

int main(int argc, char **argv) {
    // by hand
    expect(">a\nACGTA\nCGTAC\n", true, {"ACGTACGTAC"}, 15);
    expect(">a\r\nAC\r\nGT\r\n>b\n\n>c\nTT", true, {"ACGT", "", "TT"}, 21);
    expect(">a\nAC\rGT\r\r\nTT\r", true, {"AC\rGT\rTT\r"}, 14);       // a '\r' is line end only directly in front of '\n'
    expect(">a\nACG>T\n>b>c\n>\nGG\n", true, {"ACG>T", "", "GG"}, 19);  // '>' inside a line is a byte like any other
    expect(">a\n\nAC\n\n\nGT\n\n", true, {"ACGT"}, 13);
    expect(">a\nAC\n>b\nGG\nT", false, {"AC"}, 6);
    expect(">a\nAC\n>b\nGG\nT", true, {"AC", "GGT"}, 13);
    expect(">a\nAC\n>", false, {"AC"}, 6);
    expect(">a\nAC\n", false, {}, 0);                                   // one header: nothing is whole yet
    expect(">abc", false, {}, 0);
    expect(">abc", true, {""}, 4);
    expect("", true, {}, 0);
    {
        pf_fasta::Index ix;
        const Exact e("ACGT\n>a\nAC\n", 11);
        CHECK(pf_fasta::index_fasta(e.p.get(), e.n, true, ix) == pf_fasta::CLAUSE_NO_HEADER, "sequence in front of the first header is refused");
        CHECK(pf_fasta::index_fasta_words(e.p.get(), e.n, true, ix) == pf_fasta::CLAUSE_NO_HEADER, "... by the word form as well");
    }
    // every cut of texts that cross word edges every way
    std::vector<std::pair<std::string, std::string>> texts;
    for (int width : {1, 7, 59, 63, 64, 65, 127}) {
        std::string t;
        unsigned x = 12345u + (unsigned)width;
        for (int r = 0; r < 6; ++r) {
            t += ">r" + std::to_string(r) + std::string(r == 3 ? 210 : 0, 'h') + (r % 2 ? "\r\n" : "\n");
            const int len = r == 1 ? 0 : 40 + 37 * r;
            for (int i = 0; i < len; ++i) {
                x = x * 1664525u + 1013904223u;
                t += "ACGT>N"[(x >> 24) % 6];
                if ((i + 1) % width == 0 || i + 1 == len) t += r % 2 ? "\r\n" : "\n";
            }
            if (r == 4) t += "\n\n";
        }
        texts.emplace_back("width " + std::to_string(width), t);
    }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        unsigned char len4[4];
        int i = 0;
        while (fread(len4, 1, 4, f) == 4) {
            const size_t n = (size_t)len4[0] | (size_t)len4[1] << 8 | (size_t)len4[2] << 16 | (size_t)len4[3] << 24;
            std::string t(n, '\0');
            if (n && fread(&t[0], 1, n, f) != n) { fprintf(stderr, "short text in %s\n", argv[1]); return 2; }
            texts.emplace_back("text " + std::to_string(i++) + " of the file", t);
        }
        fclose(f);
    }
    for (const auto &t : texts) every_cut(t.first, t.second);
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
