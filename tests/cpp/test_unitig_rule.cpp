// Stand-alone check of csrc/pf_unitig_rule.hpp (host side only): neighbour arithmetic, the removal predicate, the default g, the
// line-length formula, and pf_unitig::build_host on the example worked by hand in tests/unitig_cases.py and on a few shapes whose text
// can be written down.  Built by tests/test_unitig_cpu.py with -fsanitize=address,undefined; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pf_unitig_rule.hpp"

static int failures = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static uint64_t enc(const std::string &s) {
    uint64_t v = 0;
    for (char c : s) v = (v << 2) | (uint64_t)(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3);
    return v;
}
static std::vector<uint64_t> kmers_of(const std::vector<std::string> &reads, int k) {
    std::vector<uint64_t> v;
    for (const std::string &r : reads)
        for (size_t i = 0; i + (size_t)k <= r.size(); ++i) v.push_back(pf_unitig::canon(enc(r.substr(i, (size_t)k)), k));
    return v;
}
static std::string body(const std::string &text) { return text.substr(text.find('\n') + 1); }

int main() {
    using namespace pf_unitig;
    // neighbours
    CHECK(succ_of(enc("ACG"), 3, 3) == enc("CGT"));
    CHECK(pred_of(enc("ACG"), 3, 3) == enc("TAC"));
    CHECK(succ_of(enc("TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT"), 0, 31) == enc("TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTA"));
    CHECK(pred_of(enc("TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT"), 1, 31) == enc("CTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT"));
    CHECK(canon(enc("CGG"), 3) == enc("CCG") && canon(enc("ACG"), 3) == enc("ACG"));
    CHECK(self_complementary(enc("ACGT"), 4) && !self_complementary(enc("ACGG"), 4) && !self_complementary(enc("ACG"), 3));
    // the predicate: (n_kmers, p, s, k, -i, -d)
    CHECK(!removed(3, 0, 0, 25, false, false));
    CHECK(removed(3, 0, 0, 25, false, true) && !removed(3, 1, 0, 25, false, true) && !removed(25, 0, 0, 25, false, true));
    CHECK(removed(3, 1, 0, 25, true, false) && removed(3, 0, 1, 25, true, false) && !removed(3, 0, 0, 25, true, false) && !removed(3, 1, 1, 25, true, false));
    CHECK(removed(3, 0, 0, 25, true, true) && removed(24, 1, 0, 25, true, true) && !removed(24, 1, 1, 25, true, true) && !removed(24, 2, 0, 25, true, true));
    CHECK(!removed(25, 1, 0, 25, true, true));
    // g, ids, lines
    CHECK(default_g(31) == 23 && default_g(25) == 17 && default_g(15) == 7 && default_g(14) == 10 && default_g(7) == 3 && default_g(6) == 4 && default_g(3) == 1);
    CHECK(g_ok(1, 3) && !g_ok(2, 3) && !g_ok(0, 25) && g_ok(23, 25) && !g_ok(24, 25));
    CHECK(id_digits(1) == 1 && id_digits(9) == 1 && id_digits(10) == 2 && id_digits(99) == 2 && id_digits(100) == 3 && id_digits(9999) == 4 && id_digits(10000) == 5);
    CHECK(line_bytes(1, 1, 3) == std::string("S\t1\tACG\n").size() && line_bytes(10, 2, 3) == std::string("S\t10\tACGG\n").size());
    CHECK(header_line(25, 17) == "H\tVN:Z:1.0\tBV:Z:1.0.6\tKL:Z:25\tML:Z:17\n");
    CHECK(base_char(0) == 'A' && base_char(1) == 'C' && base_char(2) == 'G' && base_char(7) == 'T');
    // the example worked by hand (tests/unitig_cases.py: HAND)
    {
        const std::vector<uint64_t> km = kmers_of({"AAGACTCCATG", "ACTCG", "GCGTAA"}, 5);
        Stats st;
        CHECK(body(build_host(km, 5, false, false, 3, &st)) == "S\t1\tAAGACTC\nS\t2\tACTCCATG\nS\t3\tACTCG\nS\t4\tGCGTAA\n");
        CHECK(st.distinct == 10 && st.unitigs == 4 && st.removed == 0 && st.unitigs_out == 4 && st.longest == 8);
        CHECK(body(build_host(km, 5, true, false, 3, &st)) == "S\t1\tAAGACTCCATG\nS\t2\tGCGTAA\n");
        CHECK(st.unitigs == 4 && st.removed == 1 && st.unitigs_out == 2 && st.longest == 11 && st.bytes == header_line(5, 3).size() + 27);
        CHECK(body(build_host(km, 5, false, true, 3, &st)) == "S\t1\tAAGACTC\nS\t2\tACTCCATG\nS\t3\tACTCG\n");
        CHECK(st.removed == 1 && st.unitigs_out == 3);
        CHECK(body(build_host(km, 5, true, true, 3, &st)) == "S\t1\tAAGACTCCATG\n");
        CHECK(st.removed == 2 && st.unitigs_out == 1);
    }
    // no k-mer: the header alone
    {
        Stats st;
        CHECK(build_host({}, 25, true, true, 17, &st) == header_line(25, 17) && st.unitigs_out == 0 && st.bytes == header_line(25, 17).size());
    }
    // a homopolymer: one k-mer whose only neighbour is itself
    CHECK(body(build_host(kmers_of({std::string(60, 'A')}, 25), 25, true, true, 17)) == "S\t1\t" + std::string(25, 'A') + "\n");
    // a closed cycle of seven k-mers (k = 5), read once round and k - 1 bases on
    {
        const std::string circle = "AACCGTG";   // 7 windows of 5 around it, none the reverse complement of another
        const std::string twice = circle + circle;
        const std::vector<uint64_t> km = kmers_of({twice.substr(0, 7 + 4)}, 5);
        Stats st;
        const std::string t = body(build_host(km, 5, true, true, 3, &st));
        CHECK(st.distinct == 7 && st.unitigs == 1 && st.removed == 0 && st.unitigs_out == 1 && st.longest == 11);
        CHECK(t == "S\t1\tAACCGTGAACC\n");   // starts with its smallest canonical k-mer as stored
    }
    // even k: the chain ends at the k-mer equal to its own reverse complement
    CHECK(body(build_host(kmers_of({"ACGTACGTACGTACGTACGT"}, 8), 8, false, false, 4)) == "S\t1\tACGTACGTAC\n");
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
