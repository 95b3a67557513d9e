// The shared rule header of `ploidyfrost mask` (csrc/pf_mask_rule.hpp) on its own, with plain g++ (and the sanitizers): byte classes
// over all 256 bytes, "bad set -> masked byte" against the definition for every bad set of short reads, the FASTQ index with its
// format clauses and chunk ends.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pf_mask_rule.hpp"

static int fails = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("line %d: %s\n", __LINE__, #cond);                 \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static void byte_classes() {
    const std::string bases = "ACGTacgt";
    for (int b = 0; b < 256; ++b) CHECK(pf_mask::is_base((uint8_t)b) == (bases.find((char)b) != std::string::npos && b != 0));
    const char *order = "ACGT";
    for (uint32_t c = 0; c < 4; ++c) {
        CHECK(pf_mask::base_code((uint8_t)order[c]) == c);
        CHECK(pf_mask::base_code((uint8_t)(order[c] + 32)) == c);
    }
    for (uint64_t l = 0; l < 9; ++l) CHECK(pf_mask::line_role(l) == (int)(l % 4));
    CHECK(pf_mask::line_role(5) == pf_mask::LINE_SEQUENCE && pf_mask::line_role(7) == pf_mask::LINE_QUALITY);
}

// every bad set of every read length up to 13 at k = 1, 3, 4, 5, against "byte j is masked when some bad i has i <= j < i + k"
static void bad_sets() {
    for (uint32_t k : {1u, 3u, 4u, 5u}) {
        for (uint64_t n = 0; n <= 13; ++n) {
            const uint64_t windows = n >= k ? n - k + 1 : 0;
            for (uint64_t set = 0; set < (1ull << windows); ++set) {
                std::string seq(n, 'a'), out(n, '?'), want(n, 'a');
                if (n > 2) seq[2] = want[2] = 'N';   // an input N under a bad window does not count as changed
                std::vector<uint32_t> c(windows + 1, 7);
                uint64_t changed = 0;
                for (uint64_t i = 0; i < windows; ++i)
                    if ((set >> i) & 1) c[i] = (i & 1) ? 2 : 90;   // below low, above up
                for (uint64_t j = 0; j < n; ++j) {
                    bool m = false;
                    for (uint64_t i = 0; i < windows; ++i) m |= ((set >> i) & 1) && i <= j && j < i + k;
                    if (m) { changed += want[j] != 'N'; want[j] = 'N'; }
                }
                const uint64_t got = pf_mask::mask_read(seq.data(), n, k, c.data(), 5, 50, out.data());
                CHECK(out == want && got == changed);
            }
        }
    }
    // the longest k: window j - 30 still covers byte j, window j - 31 does not
    CHECK(pf_mask::byte_masked(1ull << 33, 31) && !pf_mask::byte_masked(1ull << 32, 31) && pf_mask::byte_masked(1ull << 63, 1));
    CHECK(!pf_mask::window_bad(5, 5, 5) && pf_mask::window_bad(4, 5, 5) && pf_mask::window_bad(6, 5, 5) && !pf_mask::window_bad(0, 0, 0xFFFFFFFFu));
}

struct Index {
    int clause;
    uint64_t used, recs, bad;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
};
static Index index_of(const std::string &t, bool final) {
    Index x;
    x.clause = pf_mask::index_fastq(t.data(), t.size(), final, x.used, x.recs, x.bad, &x.off, &x.len);
    return x;
}

static void fastq_index() {
    const std::string two = "@a\nACGT\n+\nIIII\n@b\r\nAC\r\n+b\r\n@+\r\n";
    Index x = index_of(two, true);
    CHECK(x.clause == 0 && x.recs == 2 && x.used == two.size() && x.off[0] == 3 && x.len[0] == 4 && x.off[1] == 19 && x.len[1] == 2);
    x = index_of(two.substr(0, two.size() - 1), true);   // the last line without its \n: the \r is then part of the line
    CHECK(x.clause == pf_mask::CLAUSE_QUALITY && x.bad == 1);
    x = index_of("@a\nACGT\n+\nIIII", true);
    CHECK(x.clause == 0 && x.recs == 1 && x.used == 14);
    // chunk ends inside each of the four lines of the second record
    const std::string rec = "@a\nACGT\n+\nIIII\n";
    for (size_t cut : {1u, 4u, 8u, 11u, 14u}) {
        x = index_of(rec + rec.substr(0, cut), false);
        CHECK(x.clause == 0 && x.recs == 1 && x.used == rec.size());
    }
    x = index_of(rec.substr(0, 9), false);
    CHECK(x.clause == 0 && x.recs == 0 && x.used == 0);
    x = index_of("", true);
    CHECK(x.clause == 0 && x.recs == 0 && x.used == 0);
    // the clauses, each by its name, with the smallest offending record
    x = index_of(rec + "a\nACGT\n+\nIIII\n" + "@c\nAC\n-\nII\n", true);
    CHECK(x.clause == pf_mask::CLAUSE_HEADER && x.bad == 1);
    x = index_of(rec + "@a\nACGT\n-\nIIII\n", true);
    CHECK(x.clause == pf_mask::CLAUSE_PLUS && x.bad == 1);
    x = index_of(rec + rec + "@a\nACGT\n+\nIII\n", true);
    CHECK(x.clause == pf_mask::CLAUSE_QUALITY && x.bad == 2);
    x = index_of(rec + "@a\nACGT\n+\n", true);
    CHECK(x.clause == pf_mask::CLAUSE_LINE_COUNT && x.bad == 1);
    x = index_of("\n\n\n\n", true);   // an empty first line does not start with '@'
    CHECK(x.clause == pf_mask::CLAUSE_HEADER && x.bad == 0);
    const unsigned char gz[2] = {0x1f, 0x8b}, fa[2] = {'>', 's'}, fq[2] = {'@', 'r'};
    CHECK(pf_mask::file_clause(gz, 2) == pf_mask::CLAUSE_GZIP && pf_mask::file_clause(fa, 2) == pf_mask::CLAUSE_FASTA);
    CHECK(pf_mask::file_clause(fq, 2) == 0 && pf_mask::file_clause(fq, 0) == 0 && pf_mask::file_clause(gz, 1) == 0);
    for (int c = 1; c < pf_mask::CLAUSE_COUNT_; ++c) CHECK(std::string(pf_mask::clause_text(c)) != pf_mask::clause_text(0));
}

int main() {
    byte_classes();
    bad_sets();
    fastq_index();
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
