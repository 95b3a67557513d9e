// The rule of `ploidyfrost run-multi` in one place, for the kernels (pf_union.hip, k_col_keys of pf_color.hip), the host layer
// (host/pf_runmulti_host.cpp) and the host restatement: why the coloured graph and its colour sets may be made from the distinct
// k-mers of every sample's masked reads instead of from the masked reads themselves.
//
//   S_c        the sorted distinct canonical k-mers of sample c's masked reads.  A window of masked file c is valid exactly when
//              K-MASKCOUNT keeps it (pf_run_rule.hpp: survives), so S_c is what pf_count_finish(ci = 1) gives behind
//              pf_maskcount_fastq over the unmasked files of sample c with [L_c, -u].
//   vertices   `build-multi` counts the masked files of all samples together (ci = 1): the k-mers of all masked files are the union
//              of S_0 .. S_{C-1}, sorted and distinct as pf_unitig_build_colored takes them.  That union is K-UNION.
//   colours    colour c lies on graph k-mer x exactly when some valid window of masked file c has x as its canonical form
//              (pf_color_rule.hpp), i.e. exactly when x is in S_c.  A key that -i / -d removed colours nothing, from a window as
//              from a key.  Colouring per distinct key (K-COLORSET) therefore sets the planes K-COLOR sets from the windows: one
//              look-up per distinct k-mer instead of one per window, and no third read of the inputs.
//
// K-UNION merges pairwise, A before B among equal keys; a key equal to its predecessor in merged order is dropped.  Both inputs are
// distinct, so an equal pair is always one key of A followed by the same key of B and one of the two survives.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace pf_runmulti {

constexpr uint32_t MAX_SETS = 1024;   // a set is a sample is a colour (pf_color::MAX_COLORS)
constexpr int UNION_ITEMS = 4;        // merged positions a lane
constexpr int UNION_TILE = 1024;      // merged positions a block: 256 lanes of UNION_ITEMS
constexpr const char *TOO_MANY_SETS_TEXT = "more than 1024 sets";
constexpr const char *TOO_MANY_SAMPLES_TEXT = "more than 1024 samples (--sample)";

inline std::string unsorted_text(uint64_t set) { return "set " + std::to_string(set) + " is not sorted (the keys of a set ascend)"; }
inline std::string repeat_text(uint64_t set) { return "set " + std::to_string(set) + " holds a key twice (the keys of a set are distinct)"; }
// the refusal of an array that does not fit, with the counts reached
inline std::string no_room_text(const std::string &what, uint64_t need, uint64_t free_bytes, uint64_t n_a, uint64_t n_b) {
    return what + " (" + std::to_string(need) + " bytes) do not fit in the free device memory (" + std::to_string(free_bytes) + " bytes) at " +
           std::to_string(n_a) + " and " + std::to_string(n_b) + " keys";
}

// ---- the host's plain restatement (no device): what the kernel is held to ----
// one merge as the kernel defines it: merged order with A before B among equal keys, a key equal to its predecessor dropped
inline std::vector<uint64_t> union_pair_host(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) {
    std::vector<uint64_t> out;
    out.reserve(a.size() + b.size());
    size_t i = 0, j = 0;
    while (i < a.size() || j < b.size()) {
        const bool from_a = i < a.size() && (j >= b.size() || a[i] <= b[j]);
        const uint64_t key = from_a ? a[i++] : b[j++];
        if (out.empty() || out.back() != key) out.push_back(key);
    }
    return out;
}
// "" = ascending and distinct
inline std::string set_refusal(const uint64_t *keys, uint64_t n, uint64_t set) {
    bool unsorted = false, repeat = false;
    for (uint64_t i = 1; i < n; ++i) {
        unsorted = unsorted || keys[i - 1] > keys[i];
        repeat = repeat || keys[i - 1] == keys[i];
    }
    return unsorted ? unsorted_text(set) : repeat ? repeat_text(set) : "";
}
// the rounds: pairs merged, an odd set carried
inline std::vector<uint64_t> union_host(std::vector<std::vector<uint64_t>> sets) {
    if (sets.empty()) return {};
    while (sets.size() > 1) {
        std::vector<std::vector<uint64_t>> next;
        for (size_t j = 0; j + 1 < sets.size(); j += 2) next.push_back(union_pair_host(sets[j], sets[j + 1]));
        if (sets.size() & 1) next.push_back(std::move(sets.back()));
        sets.swap(next);
    }
    return sets[0];
}

}  // namespace pf_runmulti
