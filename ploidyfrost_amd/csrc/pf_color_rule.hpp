// The rule of `ploidyfrost build-multi` (K-COLOR) in one place, for the kernels (pf_unitig.hip, pf_color.hip), the host layer
// (host/pf_build_host.cpp, host/pf_bfg_write.hpp) and the stand-alone test (tests/cpp/test_bfg_write.cpp): which colours lie on which
// k-mers of the graph `build` makes from several files of reads together, where each unitig's colour set goes in <sample>.bfg_colors,
// and which `DA:Z:` tag its S line carries.  It restates what `Bifrost build -c` does behind the graph (buildUnitigColors,
// bifrost/src/ColoredCDBG.tcc:805-887; DataStorage, bifrost/src/DataStorage.tcc); keys are pf_count_rule.hpp's.
//
//   colour     colour c (the c-th file given) lies on k-mer x of the written graph when some window of some read of file c has x as its
//              canonical form.  A window is k bytes, all in ACGTacgt, as in K-COUNT.  A window whose k-mer -i / -d removed colours nothing.
//   ids        the colour set of a unitig of m k-mers is the sorted ids c * m + p, p the k-mer's position in the S line as written.  Ids
//              of adjacent colours merge into one run: colour c on the last k-mer and colour c + 1 on the first.
//   placement  nb_cs = number of S lines.  Round s = 1 .. n_seeds: every unplaced line asks for slot
//              bifrost_kmer_hash(head k-mer left-aligned, seed_of(s)) % nb_cs; a free slot goes to the smallest line that asks for it.
//              DA = the round that placed the line.  A line left over gets DA 0 and the overflow slot nb_cs + its rank among those.
//   seeds      seed_of(s) = splitmix64 of the round number: fixed, so the two files are deterministic.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "pf_unitig_rule.hpp"

namespace pf_color {

constexpr uint32_t MAX_COLORS = 1024;
constexpr uint32_t DEFAULT_SEEDS = 31;
constexpr uint32_t MAX_SEEDS = 255;   // DataStorage::read refuses 256 and more
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;
constexpr const char *TOO_MANY_COLORS_TEXT = "more than 1024 colours (-r files)";
constexpr const char *TOO_LONG_TEXT = "a unitig whose colours times k-mers reach 2^32 (ids of a colour set are 32 bits)";
constexpr const char *DA_PREFIX = "\tDA:Z:";
constexpr uint32_t DA_PREFIX_BYTES = 6;

// ---- wyhash final version 3 (public domain, github.com/wangyi-fudan/wyhash) for an 8-byte key: Kmer::hash(seed) at MAX_KMER_SIZE = 32 ----
PF_MASK_HD inline uint64_t wymix(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (a * b) ^ __umul64hi(a, b);
#else
    const __uint128_t r = (__uint128_t)a * b;
    return (uint64_t)r ^ (uint64_t)(r >> 64);
#endif
}
PF_MASK_HD inline uint64_t bifrost_kmer_hash(uint64_t x, uint64_t seed) {
    // len = 8: a = (first 4 bytes << 32) | last 4 bytes, b = (last 4 bytes << 32) | first 4 bytes, little endian
    const uint64_t wyp0 = 0xa0761d6478bd642full, wyp1 = 0xe7037ed1a0b428dbull;
    const uint64_t lo = x & 0xFFFFFFFFull, hi = x >> 32;
    const uint64_t a = (lo << 32) | hi, b = (hi << 32) | lo;
    return wymix(wyp1 ^ 8, wymix(a ^ wyp1, b ^ (seed ^ wyp0)));
}
PF_MASK_HD inline uint64_t seed_of(uint32_t round) {   // splitmix64 of the round number, 1 .. n_seeds
    uint64_t z = (uint64_t)round * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
PF_MASK_HD inline uint64_t left_aligned(uint64_t kmer, int k) { return kmer << (64 - 2 * k); }
PF_MASK_HD inline uint32_t asked_slot(uint64_t head_kmer, int k, uint32_t round, uint64_t nb_cs) {
    return (uint32_t)(bifrost_kmer_hash(left_aligned(head_kmer, k), seed_of(round)) % nb_cs);
}
PF_MASK_HD inline uint32_t da_bytes(uint32_t da) { return DA_PREFIX_BYTES + pf_unitig::id_digits(da); }   // "\tDA:Z:<n>"
inline bool seeds_ok(uint64_t n_seeds) { return n_seeds >= 1 && n_seeds <= MAX_SEEDS; }
inline std::string seeds_text() { return "the number of hash seeds goes from 1 to 255"; }
// the refusal of planes and table that do not fit, with the counts reached
inline std::string no_room_text(uint64_t need, uint64_t free_bytes, uint64_t n_colors, uint64_t n_kmers) {
    return "the colour planes and the table (" + std::to_string(need) + " bytes) do not fit in the free device memory (" + std::to_string(free_bytes) +
           " bytes) at " + std::to_string(n_colors) + " colours and " + std::to_string(n_kmers) + " k-mers of the graph";
}

typedef std::pair<uint32_t, uint32_t> Run;   // ids first .. second of one unitig's colour set

struct Line {   // one S line
    uint64_t head = 0;       // first k-mer as written, right-aligned
    uint32_t m = 0;          // k-mers
    uint32_t slot = NO_SLOT;
    uint32_t da = 0;
};
struct Stats {
    uint64_t colors = 0, windows_colored = 0, windows_unplaced = 0, windows_bad = 0, runs = 0, overflow = 0;
};
struct Colored {   // what leaves the device, and what the writer (host/pf_bfg_write.hpp) takes
    std::vector<Line> lines;
    std::vector<uint64_t> run_off;   // lines + 1 entries
    std::vector<Run> runs;
    uint64_t overflow = 0;
};

// ---- the host's plain restatement (no device, nothing tiled): what the kernels are held to ----
namespace host {

// slots and DA tags of the lines, by the rule above
inline uint64_t place(std::vector<Line> &lines, int k, uint32_t n_seeds) {
    const uint64_t nb_cs = lines.size();
    std::vector<uint32_t> owner(nb_cs, NO_SLOT);
    for (uint32_t s = 1; s <= n_seeds; ++s) {
        std::vector<uint32_t> claim(nb_cs, NO_SLOT);
        for (uint32_t j = 0; j < nb_cs; ++j) {
            if (lines[j].slot != NO_SLOT) continue;
            const uint32_t at = asked_slot(lines[j].head, k, s, nb_cs);
            if (owner[at] == NO_SLOT && claim[at] == NO_SLOT) claim[at] = j;   // (ascending j: the smallest)
        }
        for (uint32_t at = 0; at < nb_cs; ++at) {
            if (claim[at] == NO_SLOT) continue;
            owner[at] = claim[at];
            lines[claim[at]].slot = at;
            lines[claim[at]].da = s;
        }
    }
    uint64_t over = 0;
    for (Line &l : lines)
        if (l.slot == NO_SLOT) { l.slot = (uint32_t)(nb_cs + over++); l.da = 0; }
    return over;
}

// the windows of one read, as K-COUNT takes them: true = a k-mer was made
template <class F>
inline void windows(const std::string &read, int k, uint64_t &bad, F &&f) {
    for (size_t at = 0; at + (size_t)k <= read.size(); ++at) {
        uint64_t x = 0;
        bool ok = true;
        for (int b = 0; b < k && ok; ++b) {
            const uint8_t ch = (uint8_t)read[at + (size_t)b];
            ok = pf_mask::is_base(ch);
            x = (x << 2) | pf_mask::base_code(ch);
        }
        if (!ok) { ++bad; continue; }
        f(pf_unitig::canon(x, k));
    }
}

inline uint64_t encode_kmer(const char *s, int k) {
    uint64_t x = 0;
    for (int b = 0; b < k; ++b) x = (x << 2) | pf_mask::base_code((uint8_t)s[b]);
    return x;
}

}  // namespace host

// The two files from the reads of every colour: the text of <out>.gfa (pf_unitig::build_host's with the DA tags) and what the writer
// turns into <out>.bfg_colors.  reads[c] = the reads of colour c.
inline std::string build_colored_host(const std::vector<std::vector<std::string>> &reads, int k, bool clip_tips, bool del_isolated, int g, uint32_t n_seeds,
                                      Colored &out, pf_unitig::Stats *graph_stats = nullptr, Stats *stats = nullptr) {
    Stats st;
    st.colors = reads.size();
    std::vector<uint64_t> all;
    uint64_t bad = 0;
    for (const auto &file : reads)
        for (const std::string &r : file) host::windows(r, k, bad, [&](uint64_t x) { all.push_back(x); });
    pf_unitig::Stats gst;
    const std::string plain = pf_unitig::build_host(all, k, clip_tips, del_isolated, g, &gst);
    // the lines of the plain text: head, k-mers, and where every k-mer of the graph lies
    out = Colored{};
    std::map<uint64_t, std::pair<uint32_t, uint32_t>> where;   // canonical k-mer -> (line, position)
    std::vector<std::pair<size_t, size_t>> seq_at;             // (begin, end) of every sequence in `plain`
    size_t at = plain.find('\n') + 1;
    while (at < plain.size()) {
        const size_t nl = plain.find('\n', at), tab = plain.find('\t', at + 2);
        const size_t b = tab + 1, e = nl;
        Line l;
        l.m = (uint32_t)(e - b - (size_t)k + 1);
        l.head = host::encode_kmer(plain.data() + b, k);
        for (uint32_t p = 0; p < l.m; ++p) where[pf_unitig::canon(host::encode_kmer(plain.data() + b + p, k), k)] = {(uint32_t)out.lines.size(), p};
        out.lines.push_back(l);
        seq_at.emplace_back(b, e);
        at = nl + 1;
    }
    out.overflow = st.overflow = host::place(out.lines, k, n_seeds);
    // bits: per line, colour-major
    std::vector<std::vector<bool>> bits(out.lines.size());
    for (size_t j = 0; j < out.lines.size(); ++j) bits[j].assign((size_t)reads.size() * out.lines[j].m, false);
    for (size_t c = 0; c < reads.size(); ++c)
        for (const std::string &r : reads[c])
            host::windows(r, k, st.windows_bad, [&](uint64_t x) {
                const auto it = where.find(x);
                if (it == where.end()) { ++st.windows_unplaced; return; }
                ++st.windows_colored;
                bits[it->second.first][c * (size_t)out.lines[it->second.first].m + it->second.second] = true;
            });
    for (size_t j = 0; j < out.lines.size(); ++j) {
        out.run_off.push_back(out.runs.size());
        for (size_t id = 0; id < bits[j].size(); ++id) {
            if (!bits[j][id]) continue;
            if (id && bits[j][id - 1]) out.runs.back().second = (uint32_t)id;
            else out.runs.emplace_back((uint32_t)id, (uint32_t)id);
        }
    }
    out.run_off.push_back(out.runs.size());
    st.runs = out.runs.size();
    // the text with the tags
    std::string text = plain.substr(0, plain.find('\n') + 1);
    for (size_t j = 0; j < out.lines.size(); ++j)
        text += "S\t" + std::to_string(j + 1) + "\t" + plain.substr(seq_at[j].first, seq_at[j].second - seq_at[j].first) + DA_PREFIX + std::to_string(out.lines[j].da) + "\n";
    gst.bytes = text.size();
    if (graph_stats) *graph_stats = gst;
    if (stats) *stats = st;
    return text;
}

}  // namespace pf_color
