// The rule of `ploidyfrost build` (K-UNITIG) in one place, for the kernels (pf_unitig.hip), the host layer (host/pf_build_host.cpp) and
// the stand-alone test (tests/cpp/test_unitig_rule.cpp): which compacted de Bruijn graph the sorted distinct canonical k-mers of the
// reads (what pf_count_finish leaves on the device) make, and how it is written.  It restates what step `4.bifrost` of the reference's
// workflow asks of `Bifrost build [-i] [-d] -k <k> -r reads.fq -o sample`; keys are pf_count_rule.hpp's (A0 C1 G2 T3, first base most
// significant, canonical = min(fw, rc)).
//
//   vertices   S = the canonical k-mers.  succ(x) = the x[1:] + b, b in ACGT, whose canonical form is in S; pred(x) the same in front.
//   link       an oriented k-mer x links to y when succ(x) == [y], pred(y) == [x] and canon(x) != canon(y).  A unitig is a maximal chain
//              of links that visits no canonical k-mer twice.  (Only a k-mer equal to its own reverse complement -- even k -- can make a
//              chain come back to a k-mer it holds: both of its sides lead to the same neighbour, and the chain ends at it.)
//   simplify   CompactedDBG::removeUnitigs (-i clip tips, -d delete isolated): every unitig of fewer than k k-mers is decided against the
//              graph as it stands by removed(), deletion comes afterwards: the result does not depend on order.
//   recompact  the link rule once more over S minus the k-mers of the removed unitigs; one pass, not a fixed point.
//   output     H line (KL = k, ML = g), then one `S <id> <sequence>` line per unitig, ids 1 .. N, no L lines.  A unitig is written in the
//              reading whose first k-mer, as read, is the smaller one; a closed cycle starts with its smallest canonical k-mer in
//              canonical form; lines ascend by their first k-mer as read.
//
// PARITY: pinned against the reference's Bifrost 1.0.6 under tests/unitig_cases.py's comparator (tests/golden/build_*).  One known
// difference: a closed walk through two self-complementary k-mers (`ACGT` repeated, k = 8) is written by Bifrost with four k-mers, the
// fourth the reverse complement of the second; here it ends at the third, as the link rule says.
#pragma once
#include <stdint.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "pf_count_rule.hpp"

namespace pf_unitig {

constexpr uint64_t MAX_KMERS = 1ull << 31;   // oriented k-mers are numbered 2 i + o in 32 bits
constexpr const char *TOO_MANY_TEXT = "2^31 or more distinct k-mers (oriented k-mers are numbered in 32 bits)";

// ---- neighbours ----
PF_MASK_HD inline uint64_t kmer_mask(int k) { return (1ull << (2 * k)) - 1; }
PF_MASK_HD inline uint64_t succ_of(uint64_t x, int b, int k) { return ((x << 2) | (uint64_t)b) & kmer_mask(k); }
PF_MASK_HD inline uint64_t pred_of(uint64_t x, int b, int k) { return (x >> 2) | ((uint64_t)b << (2 * (k - 1))); }
PF_MASK_HD inline uint64_t canon(uint64_t x, int k) { return pf_count::window_key(x, k, true); }
PF_MASK_HD inline bool self_complementary(uint64_t x, int k) { return pf_count::rev_comp(x, k) == x; }

// ---- simplify: CompactedDBG::removeUnitigs on one unitig of n_kmers k-mers with p = |pred(first)|, s = |succ(last)| ----
PF_MASK_HD inline bool removed(uint64_t n_kmers, int p, int s, int k, bool clip_tips, bool del_isolated) {
    if (n_kmers >= (uint64_t)k) return false;
    const int lim = clip_tips ? 1 : 0;
    if (p > lim || s > lim) return false;
    if (clip_tips && del_isolated) return p + s <= lim;
    if (clip_tips || del_isolated) return p + s == lim;
    return false;
}

// ---- output ----
inline int default_g(int k) { return k >= 15 ? k - 8 : k >= 7 ? k - 4 : k - 2; }   // Bifrost's minimizer length when -g is not given
inline bool g_ok(int64_t g, int k) { return g >= 1 && g <= k - 2; }
inline std::string g_text(int k) { return "-g goes from 1 to k - 2 = " + std::to_string(k - 2) + " (the minimizer length the header's ML tag names)"; }
// the refusal of buffers that do not fit, with the k-mer count reached
inline std::string no_room_text(uint64_t need, uint64_t free_bytes, uint64_t n_kmers) {
    return "the buffers of the graph (" + std::to_string(need) + " bytes) do not fit in the free device memory (" + std::to_string(free_bytes) +
           " bytes) at " + std::to_string(n_kmers) + " distinct k-mers";
}
inline std::string header_line(int k, int g) {
    return "H\tVN:Z:1.0\tBV:Z:1.0.6\tKL:Z:" + std::to_string(k) + "\tML:Z:" + std::to_string(g) + "\n";
}
PF_MASK_HD inline uint32_t id_digits(uint64_t id) {
    uint32_t d = 1;
    while (id >= 10) { id /= 10; ++d; }
    return d;
}
// bytes of "S\t<id>\t<sequence>\n" for a unitig of n_kmers k-mers
PF_MASK_HD inline uint64_t line_bytes(uint64_t id, uint64_t n_kmers, int k) { return 2 + id_digits(id) + 1 + (n_kmers + (uint64_t)k - 1) + 1; }
PF_MASK_HD inline char base_char(uint64_t code) { return (char)((0x54474341u >> (8u * ((uint32_t)code & 3u))) & 0xFFu); }   // "ACGT"[code] in a register

struct Stats {
    uint64_t distinct = 0, unitigs = 0, removed = 0, unitigs_out = 0, longest = 0, bytes = 0;
};

// ---- the host's plain restatement (no device, nothing tiled): what the kernels are held to ----
namespace host {

typedef std::set<uint64_t> Set;   // canonical k-mers
typedef std::vector<uint64_t> Chain;   // oriented k-mers

inline std::vector<uint64_t> succ(const Set &S, uint64_t x, int k) {
    std::vector<uint64_t> v;
    for (int b = 0; b < 4; ++b)
        if (S.count(canon(succ_of(x, b, k), k))) v.push_back(succ_of(x, b, k));
    return v;
}
inline std::vector<uint64_t> pred(const Set &S, uint64_t x, int k) {
    std::vector<uint64_t> v;
    for (int b = 0; b < 4; ++b)
        if (S.count(canon(pred_of(x, b, k), k))) v.push_back(pred_of(x, b, k));
    return v;
}
// the k-mer x links to; false: none
inline bool link(const Set &S, uint64_t x, int k, uint64_t &y) {
    const std::vector<uint64_t> su = succ(S, x, k);
    if (su.size() != 1 || canon(su[0], k) == canon(x, k)) return false;
    const std::vector<uint64_t> pr = pred(S, su[0], k);
    if (pr.size() != 1 || pr[0] != x) return false;
    y = su[0];
    return true;
}
struct Unitig { Chain chain; bool closed = false; };
inline std::vector<Unitig> unitigs(const Set &S, int k) {
    std::vector<Unitig> out;
    Set seen;
    for (const uint64_t c : S) {
        if (seen.count(c)) continue;
        Unitig u;
        Set inside = {c};
        u.chain.push_back(c);
        uint64_t x = c, y = 0;
        while (link(S, x, k, y)) {
            if (y == u.chain.front()) { u.closed = true; break; }
            if (inside.count(canon(y, k))) break;
            u.chain.push_back(y);
            inside.insert(canon(y, k));
            x = y;
        }
        x = c;
        while (!u.closed && link(S, pf_count::rev_comp(x, k), k, y) && !inside.count(canon(y, k))) {
            x = pf_count::rev_comp(y, k);
            u.chain.insert(u.chain.begin(), x);
            inside.insert(canon(x, k));
        }
        seen.insert(inside.begin(), inside.end());
        out.push_back(u);
    }
    return out;
}
// the reading that is written: the oriented k-mers in their order
inline Chain oriented(const Unitig &u, int k) {
    Chain c = u.chain;
    auto flip = [&](Chain &v) {
        Chain r;
        for (size_t i = v.size(); i-- > 0;) r.push_back(pf_count::rev_comp(v[i], k));
        v = r;
    };
    if (u.closed) {
        size_t j = 0;
        for (size_t i = 1; i < c.size(); ++i)
            if (canon(c[i], k) < canon(c[j], k)) j = i;
        if (c[j] != canon(c[j], k)) { flip(c); j = c.size() - 1 - j; }
        Chain r(c.begin() + (long)j, c.end());
        r.insert(r.end(), c.begin(), c.begin() + (long)j);
        c = r;
    } else if (pf_count::rev_comp(c.back(), k) < c.front()) {
        flip(c);
    }
    return c;
}
inline std::string sequence(const Chain &c, int k) {
    std::string s;
    for (int i = k - 1; i >= 0; --i) s.push_back(base_char(c[0] >> (2 * i)));
    for (size_t i = 1; i < c.size(); ++i) s.push_back(base_char(c[i]));
    return s;
}

}  // namespace host

// the text of <out>.gfa from the canonical k-mers (any order, duplicates allowed)
inline std::string build_host(const std::vector<uint64_t> &kmers, int k, bool clip_tips, bool del_isolated, int g, Stats *stats = nullptr) {
    host::Set S(kmers.begin(), kmers.end());
    Stats st;
    st.distinct = S.size();
    std::vector<host::Unitig> us = host::unitigs(S, k);
    st.unitigs = us.size();
    host::Set gone;
    for (const host::Unitig &u : us) {
        const int p = (int)host::pred(S, u.chain.front(), k).size(), s = (int)host::succ(S, u.chain.back(), k).size();
        if (!removed(u.chain.size(), p, s, k, clip_tips, del_isolated)) continue;
        st.removed += 1;
        for (const uint64_t x : u.chain) gone.insert(canon(x, k));
    }
    if (!gone.empty()) {
        for (const uint64_t x : gone) S.erase(x);
        us = host::unitigs(S, k);
    }
    std::map<uint64_t, std::string> lines;   // by the first k-mer as read
    for (const host::Unitig &u : us) {
        const host::Chain c = host::oriented(u, k);
        lines[c[0]] = host::sequence(c, k);
    }
    std::string text = header_line(k, g);
    uint64_t id = 0;
    for (const auto &kv : lines) {
        text += "S\t" + std::to_string(++id) + "\t" + kv.second + "\n";
        if (kv.second.size() > st.longest) st.longest = kv.second.size();
    }
    st.unitigs_out = id;
    st.bytes = text.size();
    if (stats) *stats = st;
    return text;
}

}  // namespace pf_unitig
