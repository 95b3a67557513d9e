// The colour rule and the writer of <sample>.bfg_colors alone (csrc/pf_color_rule.hpp, csrc/host/pf_bfg_write.hpp), host code under the
// sanitizers: plain g++ -fsanitize=address,undefined, nothing of it loaded into Python or run on a GPU.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "host/pf_bfg_write.hpp"
#include "pf_color_rule.hpp"

#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                \
        }                                                           \
    } while (0)

static std::string rand_seq(std::mt19937 &rng, size_t n) {
    std::string s;
    for (size_t i = 0; i < n; ++i) s.push_back("ACGT"[rng() & 3]);
    return s;
}

// the ids of one encoded set, decoded by hand (each form the writer has)
static std::vector<uint32_t> decode(const std::vector<uint8_t> &b, size_t &at) {
    std::vector<uint32_t> ids;
    uint64_t w;
    memcpy(&w, b.data() + at, 8);
    at += 8;
    if ((w & 7) == 1) {
        for (uint32_t i = 0; i < 61; ++i)
            if ((w >> (3 + i)) & 1) ids.push_back(i);
    } else if ((w & 7) == 2) {
        ids.push_back((uint32_t)(w >> 3));
    } else if ((w & 7) == 0) {
        uint16_t h[3];
        memcpy(h, b.data() + at, 6);
        CHECK((h[0] & 7) == 4 && (h[0] >> 3) == h[1] + 3 && h[1] % 2 == 0);
        at += 6;
        for (uint32_t i = 0; i < h[1]; i += 2) {
            uint16_t p[2];
            memcpy(p, b.data() + at, 4);
            at += 4;
            CHECK(p[0] <= p[1]);
            for (uint32_t v = p[0]; v <= p[1]; ++v) ids.push_back(((uint32_t)h[2] << 16) | v);
        }
    } else {
        CHECK((w & 7) == 3);
        const size_t end = at + (size_t)(w >> 3);
        uint32_t cookie;
        memcpy(&cookie, b.data() + at, 4);
        CHECK((cookie & 0xFFFF) == 12347);
        const uint32_t n = (cookie >> 16) + 1;
        size_t p = at + 4 + (n + 7) / 8;
        std::vector<uint16_t> keys(n);
        for (uint32_t i = 0; i < n; ++i) memcpy(&keys[i], b.data() + p + 4 * i, 2);
        p += 4 * (size_t)n;
        if (n >= 4) p += 4 * (size_t)n;
        for (uint32_t i = 0; i < n; ++i) {
            uint16_t nr;
            memcpy(&nr, b.data() + p, 2);
            p += 2;
            for (uint32_t r = 0; r < nr; ++r) {
                uint16_t sl[2];
                memcpy(sl, b.data() + p, 4);
                p += 4;
                for (uint32_t v = sl[0]; v <= (uint32_t)sl[0] + sl[1]; ++v) ids.push_back(((uint32_t)keys[i] << 16) | v);
            }
        }
        CHECK(p == end);
        at = end;
    }
    return ids;
}

static void round_trip(const std::vector<pf_color::Run> &runs) {
    std::vector<uint8_t> b;
    pf_bfg::encode_set(runs.data(), runs.size(), b);
    size_t at = 0;
    const std::vector<uint32_t> ids = decode(b, at);
    CHECK(at == b.size());
    std::vector<uint32_t> want;
    for (const pf_color::Run &r : runs)
        for (uint64_t v = r.first; v <= r.second; ++v) want.push_back((uint32_t)v);
    CHECK(ids == want);
}

int main() {
    // ---- the seeds: the first two outputs of splitmix64 from state 0, as published with the generator ----
    CHECK(pf_color::seed_of(1) == 0xE220A8397B1DCDAFull && pf_color::seed_of(2) == 0x6E789E6AA1B965F4ull);
    CHECK(pf_color::da_bytes(0) == 7 && pf_color::da_bytes(31) == 8 && pf_color::da_bytes(255) == 9);
    // ---- set forms at their borders ----
    round_trip({});
    round_trip({{0, 0}});
    round_trip({{60, 60}});
    round_trip({{61, 61}});
    round_trip({{0, 59}});
    round_trip({{0, 60}});
    round_trip({{0, 61}});
    round_trip({{3, 9}, {40, 60}});
    round_trip({{65530, 65540}});
    round_trip({{0, 21845}, {21846, 65537}});
    round_trip({{100, 299999}});
    {
        std::vector<pf_color::Run> many, more;
        for (uint32_t i = 0; i < 2046; ++i) many.emplace_back(100 + 2 * i, 100 + 2 * i);
        round_trip(many);
        for (uint32_t i = 0; i < 2047; ++i) more.emplace_back(100 + 2 * i, 100 + 2 * i);
        round_trip(more);
        std::vector<uint8_t> a, b;
        pf_bfg::encode_set(many.data(), many.size(), a);
        pf_bfg::encode_set(more.data(), more.size(), b);
        CHECK((a[0] & 7) == 0 && (b[0] & 7) == 3);   // the run-length TinyBitmap holds 2046 runs, the next one is a Roaring bitmap
    }
    // ---- the restatement: graph, placement, runs, file ----
    std::mt19937 rng(7);
    const int k = 11;
    const std::string g = rand_seq(rng, 300);
    std::string h = g;
    h[150] = h[150] == 'A' ? 'C' : 'A';
    std::vector<std::vector<std::string>> reads(3);
    for (size_t i = 0; i + 40 <= g.size(); i += 20) {
        reads[0].push_back(g.substr(i, 40));
        reads[1].push_back(h.substr(i, 40));
    }
    reads[1].push_back(g.substr(40, 10) + "T");   // a tip, most likely
    reads[2].push_back("acgtn");
    for (int flags = 0; flags < 4; ++flags) {
        for (uint32_t n_seeds : {1u, 31u}) {
            pf_color::Colored cg;
            pf_unitig::Stats gst;
            pf_color::Stats cst;
            const std::string text = pf_color::build_colored_host(reads, k, flags & 1, flags & 2, pf_unitig::default_g(k), n_seeds, cg, &gst, &cst);
            CHECK(gst.bytes == text.size() && cg.lines.size() == gst.unitigs_out && cg.run_off.size() == cg.lines.size() + 1);
            CHECK(cst.colors == 3 && cst.runs == cg.runs.size() && cst.overflow == cg.overflow && cst.windows_colored > 0);
            uint64_t zeros = 0;
            std::vector<bool> taken(cg.lines.size() + cg.overflow, false);
            for (const pf_color::Line &l : cg.lines) {
                CHECK(l.slot < taken.size() && !taken[l.slot]);
                taken[l.slot] = true;
                CHECK((l.da == 0) == (l.slot >= cg.lines.size()));
                if (l.da) CHECK(pf_color::asked_slot(l.head, k, l.da, cg.lines.size()) == l.slot);
                zeros += l.da == 0;
            }
            CHECK(zeros == cg.overflow);
            std::vector<uint8_t> bytes;
            CHECK(pf_bfg::write(cg, k, n_seeds, {"a.fq", "b.fq", "c.fq"}, bytes).empty());
            uint64_t head[7];
            memcpy(head, bytes.data(), sizeof head);
            CHECK(head[0] == 2 && head[1] == n_seeds && head[2] == 3 && head[3] == cg.lines.size() && head[4] == cg.lines.size() + cg.overflow &&
                  head[5] == 0 && head[6] == cg.overflow);
            // the sets, read back in slot order from the first block offset
            const size_t pos_at = 7 * 8 + 8 * (size_t)n_seeds + 8;
            int64_t first = 0;
            if (head[4]) memcpy(&first, bytes.data() + pos_at, 8);
            size_t at = head[4] ? (size_t)first : bytes.size();
            std::vector<uint32_t> owner(taken.size(), pf_color::NO_SLOT);
            for (size_t j = 0; j < cg.lines.size(); ++j) owner[cg.lines[j].slot] = (uint32_t)j;
            for (size_t s = 0; s < owner.size(); ++s) {
                if (s && s % 1024 == 0) {
                    int64_t p;
                    memcpy(&p, bytes.data() + pos_at + 16 * (s / 1024), 8);
                    CHECK((size_t)p == at);
                }
                const std::vector<uint32_t> ids = decode(bytes, at);
                std::vector<uint32_t> want;
                if (owner[s] != pf_color::NO_SLOT)
                    for (uint64_t r = cg.run_off[owner[s]]; r < cg.run_off[owner[s] + 1]; ++r)
                        for (uint32_t v = cg.runs[r].first; v <= cg.runs[r].second; ++v) want.push_back(v);
                CHECK(ids == want);
            }
            CHECK(at + 24 * cg.overflow == bytes.size());
        }
    }
    // a writer refuses what is no placement
    {
        pf_color::Colored bad;
        bad.lines.resize(2);
        bad.lines[0].slot = bad.lines[1].slot = 0;
        bad.run_off = {0, 0, 0};
        std::vector<uint8_t> bytes;
        CHECK(!pf_bfg::write(bad, 11, 31, {"a"}, bytes).empty());
    }
    printf("ok\n");
    return 0;
}
