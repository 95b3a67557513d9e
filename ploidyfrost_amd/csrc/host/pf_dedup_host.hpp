// `--dedup [--dedup-bases N] [--dedup-initial-slots N]` of `trim`, `run` and `run-multi`: the host side of K-DEDUP (pf_dedup_begin ..
// pf_dedup_end in ploidyfrost_hip.h, the rule in ../pf_dedup_rule.hpp) -- the options, the dedup opened on a context for one unit of a
// command (one `trim` command of the equivalent chain), its statistics fetched and worded, and the plain host restatement of the
// decision over the keys of a whole stream.
#pragma once
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../pf_clip_rule.hpp"
#include "../pf_dedup_rule.hpp"
#include "../pf_mask_rule.hpp"
#include "../pf_trim_rule.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

struct DedupOptions {
    bool on = false;
    uint32_t bases = 0;           // --dedup-bases: 0 = the whole read
    uint64_t initial_slots = 0;   // --dedup-initial-slots: 0 = the default
};
// what is refused about the options before a device context exists ("" = none)
inline std::string dedup_options_refusal(const DedupOptions &opt) {
    if (opt.on && !pf_dedup::bases_ok(opt.bases)) return "--dedup-bases takes 16 to 4096, not " + std::to_string(opt.bases);
    return "";
}
// the `dedup:` line of a unit on stderr
inline std::string dedup_line(const pf_dedup_stats &s) {
    std::string l = "dedup: units " + std::to_string(s.units) + " unique " + std::to_string(s.unique) + " duplicates " + std::to_string(s.duplicates) +
                    " max_copies " + std::to_string(s.max_copies) + " levels";
    for (uint32_t i = 0; i < pf_dedup::LEVELS; ++i) l += ' ' + std::to_string(s.levels[i]);
    return l;
}
// a fresh dedup for a unit; its statistics when the unit has streamed (stats null: no pass over the table), and the table freed.
// PF_OK, or pf_last_error(ctx) says why
inline int dedup_open(pf_ctx *ctx, const DedupOptions &opt) { return opt.on ? pf_dedup_begin(ctx, opt.bases, opt.initial_slots) : (int)PF_OK; }
inline int dedup_close(pf_ctx *ctx, const DedupOptions &opt, pf_dedup_stats *stats) {
    if (!opt.on) return PF_OK;
    if (!stats) return pf_dedup_end(ctx);
    pf_dedup_stats s = {};
    const int rc = pf_dedup_stats_get(ctx, &s);
    if (rc != PF_OK) return rc;   // (the table goes with the context)
    *stats = s;
    return pf_dedup_end(ctx);
}

// The decision restated on the host: the keys (two words each, a zero word counts as 1) of the units of a whole stream in order,
// participates[i] != 0 (null: all take part); keep[i] = 1 for a unit that takes part and is the first of its key, 0 for a later copy,
// and 1 for a unit that does not take part (nothing about it changes).  `seen` carries the keys from one call to the next.
struct DedupKey {
    uint64_t h1, h2;
    bool operator==(const DedupKey &o) const { return h1 == o.h1 && h2 == o.h2; }
};
struct DedupKeyHash {
    size_t operator()(const DedupKey &k) const { return (size_t)(k.h1 ^ (k.h2 * 0x9E3779B97F4A7C15ull)); }
};
using DedupSeen = std::unordered_map<DedupKey, uint64_t, DedupKeyHash>;   // key -> copies
inline void dedup_units(DedupSeen &seen, const uint64_t *keys, const uint8_t *participates, uint64_t n, uint8_t *keep) {
    for (uint64_t i = 0; i < n; ++i) {
        if (participates && !participates[i]) { if (keep) keep[i] = 1; continue; }
        const DedupKey k{pf_dedup::nonzero(keys[2 * i]), pf_dedup::nonzero(keys[2 * i + 1])};
        const uint64_t copies = ++seen[k];
        if (keep) keep[i] = copies == 1 ? 1 : 0;
    }
}
inline pf_dedup_stats dedup_stats_of(const DedupSeen &seen) {
    pf_dedup_stats s = {};
    for (const auto &kv : seen) {
        s.units += kv.second;
        s.unique += 1;
        if (kv.second > s.max_copies) s.max_copies = kv.second;
        s.levels[pf_dedup::level_of(kv.second)] += 1;
    }
    s.duplicates = s.units - s.unique;
    return s;
}


// What pf_trim_fastq (n_files = 1) / pf_trim_fastq_pair (2) give for one chunk with a dedup open and no clip, restated on the host: the
// index of pf_mask::index_fastq per file (its clause is returned, with bad_record; nothing is written and `seen` stays as it was),
// every whole record trimmed, every unit that takes part keyed from its raw sequence line(s) and held against `seen`, the kept ones
// appended to out (1 or 4: o1 u1 o2 u2).  begin / len: per file one entry per record, len 0 = dropped; keys (may be null): two words
// per unit, 0 0 for one that takes no part.  steps may be none.
inline int dedup_trim_chunk(int n_files, const char *const *text, const uint64_t *n, bool final, const pf_trim::Step *steps, uint32_t n_steps, uint32_t phred,
                            uint32_t bases, DedupSeen &seen, std::string *out, uint64_t *bytes_used, uint64_t &n_records, uint64_t &bad_record,
                            std::vector<uint32_t> *begin, std::vector<uint32_t> *len, pf_trim::Stats *stats, std::vector<uint64_t> *keys) {
    n_records = 0;
    bad_record = 0;
    if (keys) keys->clear();
    std::vector<uint64_t> lb[2], le[2];
    uint64_t used[2] = {0, 0}, recs[2] = {0, 0};
    for (int f = 0; f < n_files; ++f) {
        bytes_used[f] = 0;
        begin[f].clear();
        len[f].clear();
        stats[f] = pf_trim::Stats{};
        uint64_t bad = 0;
        const int clause = pf_mask::index_fastq(text[f], n[f], final, used[f], recs[f], bad);
        if (clause) { bad_record = n_files == 2 ? 2 * bad + (uint64_t)f : bad; return clause; }
        pf_trim::record_lines(text[f], used[f], recs[f], lb[f], le[f]);
    }
    uint64_t nr = recs[0];
    if (n_files == 2) {
        nr = recs[0] < recs[1] ? recs[0] : recs[1];
        if (final && recs[0] != recs[1]) { bad_record = 2 * nr + (recs[0] < recs[1] ? 0 : 1); return pf_clip::PAIR_COUNTS_DIFFER; }
    }
    for (uint64_t r = 0; r < nr; ++r) {
        uint32_t nq[2] = {0, 0}, b[2] = {0, 0}, e[2] = {0, 0};
        bool kept[2] = {false, true};
        for (int f = 0; f < n_files; ++f) {
            nq[f] = (uint32_t)(le[f][4 * r + 3] - lb[f][4 * r + 3]);
            kept[f] = pf_trim::trim_read(text[f] + lb[f][4 * r + 3], nq[f], steps, n_steps, phred, b[f], e[f]);
        }
        uint64_t key[2] = {0, 0};
        if (kept[0] && kept[1]) {   // the unit takes part
            const uint32_t n1 = (uint32_t)(le[0][4 * r + 1] - lb[0][4 * r + 1]), n2 = n_files == 2 ? (uint32_t)(le[1][4 * r + 1] - lb[1][4 * r + 1]) : 0u;
            pf_dedup::key_of(text[0] + lb[0][4 * r + 1], n1, n_files == 2 ? text[1] + lb[1][4 * r + 1] : nullptr, n2, n_files == 2, bases, key);
            uint8_t keep = 1;
            dedup_units(seen, key, nullptr, 1, &keep);
            if (!keep)
                for (int f = 0; f < n_files; ++f) { kept[f] = false; b[f] = e[f] = 0; }
        }
        if (keys) { keys->push_back(key[0]); keys->push_back(key[1]); }
        for (int f = 0; f < n_files; ++f) {
            const bool other = n_files == 2 ? kept[1 - f] : true;
            if (kept[f]) pf_trim::append_record(out[n_files == 2 ? 2 * f + (other ? 0 : 1) : 0], text[f], &lb[f][4 * r], &le[f][4 * r], b[f], e[f]);
            begin[f].push_back(b[f]);
            len[f].push_back(e[f] - b[f]);
            pf_trim::Stats &st = stats[f];
            st.reads += 1;
            st.kept += kept[f];
            st.dropped += !kept[f];
            st.bases += nq[f];
            st.bases_kept += e[f] - b[f];
            if (n_files == 2) {
                st.both += kept[0] && kept[1];
                st.only1 += kept[0] && !kept[1];
                st.only2 += !kept[0] && kept[1];
                st.neither += !kept[0] && !kept[1];
            }
        }
    }
    for (int f = 0; f < n_files; ++f) bytes_used[f] = nr < recs[f] ? lb[f][4 * nr] : used[f];
    n_records = nr;
    return pf_mask::CLAUSE_NONE;
}

}  // namespace pfh
