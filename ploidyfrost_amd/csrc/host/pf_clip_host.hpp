// `--adapters FILE [--adapter-seed S] [--adapter-score T]`: the host side of K-CLIP (pf_clip_begin .. pf_clip_end in ploidyfrost_hip.h, the
// rule in ../pf_clip_rule.hpp) for `trim`, `run` and `run-multi` -- the options, the adapter file read and refused before a device
// context exists, the clip opened on a context, and the line that reports it.  With `--adapter-pairs [--adapter-pair-score T]
// [--adapter-pair-min A] [--adapter-keep-both]` the file's Prefix entries become prefix pairs and K-PALIN runs beside K-CLIP on pairs.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../pf_clip_rule.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

struct ClipOptions {
    std::string adapters;   // "" = no clipping
    uint32_t seed = pf_clip::DEFAULT_SEED, score = pf_clip::DEFAULT_SCORE;
    bool pairs = false;     // --adapter-pairs: palindrome mode on -1 / -2
    uint32_t pair_score = pf_clip::DEFAULT_PAIR_SCORE, pair_min = pf_clip::DEFAULT_PAIR_MIN;
    bool keep_both = false;
    bool on() const { return !adapters.empty(); }
};
struct ClipReport {   // what the `clip:` line says
    uint32_t adapters = 0, skipped = 0;
    pf_clip_stats stats = {};
    bool pairs_on = false;   // --adapter-pairs: the line also holds the prefix pairs and what K-PALIN counted
    uint32_t pairs = 0;
    pf_clip_pair_stats pair_stats = {};
};
// what a clip has counted, both records (pair: zero without prefix pairs)
struct ClipCounts {
    pf_clip_stats clip = {};
    pf_clip_pair_stats pair = {};
};

// The file of opt.adapters read and parsed, seed and score checked: 0 = ok, else worded in err without the sub-command's name
// ("adapters <path>: record 3: an adapter holds 16 to 128 bases").  No device is touched.
inline int clip_load(const ClipOptions &opt, pf_clip::Adapters &A, std::string &err) {
    A.clear();
    { const int c = pf_clip::params_clause(opt.seed, opt.score); if (c) { err = pf_clip::refusal_text(c); return c; } }
    if (opt.pairs) { const int c = pf_clip::pair_params_clause(opt.pair_score, opt.pair_min); if (c) { err = pf_clip::refusal_text(c); return c; } }
    FILE *f = fopen(opt.adapters.c_str(), "rb");
    if (!f) { err = "adapters " + opt.adapters + ": cannot be opened"; return -1; }
    std::string text;
    char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) {
        text.append(buf, got);
        if (text.size() > (64u << 20)) break;   // (64 usable adapters of 128 bases: a file of this size is no adapter file)
    }
    fclose(f);
    uint64_t bad = 0;
    const int c = text.size() > (64u << 20) ? (int)pf_clip::REFUSE_NOT_FASTA : pf_clip::parse_adapters(text.data(), text.size(), A, &bad, opt.pairs);
    if (c) { err = pf_clip::file_refusal(opt.adapters, c, bad); return c; }
    return 0;
}
// the clip opened on the context: PF_OK, or the ABI's code with pf_last_error
inline int clip_open(pf_ctx *ctx, const pf_clip::Adapters &A, const ClipOptions &opt) {
    if (opt.pairs)
        return pf_clip_begin_pairs(ctx, A.bases.data(), A.off.data(), A.side.data(), A.size(), A.prefix_bases.data(), A.prefix_off.data(), A.pairs(), opt.seed,
                                   opt.score, opt.pair_score, opt.pair_min, opt.keep_both ? 1 : 0);
    return pf_clip_begin(ctx, A.bases.data(), A.off.data(), A.side.data(), A.size(), opt.seed, opt.score);
}
inline std::string clip_line(const ClipReport &r) {
    auto n = [](uint64_t v) { return std::to_string(v); };
    const pf_clip_stats &s = r.stats;
    const std::string tail = " skipped " + n(r.skipped) + " reads_clipped " + n(s.reads_clipped[0] + s.reads_clipped[1]) + " dropped " +
                             n(s.reads_dropped[0] + s.reads_dropped[1]) + " bases_clipped " + n(s.bases_clipped[0] + s.bases_clipped[1]);
    if (!r.pairs_on) return "clip: adapters " + n(r.adapters) + tail;
    const pf_clip_pair_stats &q = r.pair_stats;
    return "clip: adapters " + n(r.adapters) + " pairs " + n(r.pairs) + tail + " pairs_clipped " + n(q.pairs_clipped) + " pairs_dropped " + n(q.pairs_dropped) +
           " pairs_too_long " + n(q.pairs_too_long);
}
// what the open clip has counted since its begin (pairs: it was opened with prefix pairs)
inline int clip_counts(pf_ctx *ctx, bool pairs, ClipCounts &now) {
    now = ClipCounts{};
    const int rc = pf_clip_stats_get(ctx, &now.clip);
    if (rc != PF_OK || !pairs) return rc;
    return pf_clip_pair_stats_get(ctx, &now.pair);
}
// now - before
inline ClipCounts clip_counts_since(const ClipCounts &now, const ClipCounts &before) {
    ClipCounts d;
    for (int f = 0; f < 2; ++f) {
        d.clip.reads_clipped[f] = now.clip.reads_clipped[f] - before.clip.reads_clipped[f];
        d.clip.reads_dropped[f] = now.clip.reads_dropped[f] - before.clip.reads_dropped[f];
        d.clip.bases_clipped[f] = now.clip.bases_clipped[f] - before.clip.bases_clipped[f];
        d.clip.candidates_scored[f] = now.clip.candidates_scored[f] - before.clip.candidates_scored[f];
        d.pair.bases_clipped[f] = now.pair.bases_clipped[f] - before.pair.bases_clipped[f];
    }
    d.pair.pairs_clipped = now.pair.pairs_clipped - before.pair.pairs_clipped;
    d.pair.pairs_dropped = now.pair.pairs_dropped - before.pair.pairs_dropped;
    d.pair.pairs_too_long = now.pair.pairs_too_long - before.pair.pairs_too_long;
    d.pair.candidates_scored = now.pair.candidates_scored - before.pair.candidates_scored;
    return d;
}
// the report of one unit from what the clip counted over it
inline ClipReport clip_report_of(const pf_clip::Adapters &A, const ClipOptions &opt, const ClipCounts &c) {
    ClipReport r;
    r.adapters = A.size();
    r.skipped = A.skipped;
    r.stats = c.clip;
    r.pairs_on = opt.pairs;
    r.pairs = A.pairs();
    r.pair_stats = c.pair;
    return r;
}
// the clip's statistics since its begin into the report
inline int clip_report(pf_ctx *ctx, const pf_clip::Adapters &A, const ClipOptions &opt, ClipReport &r) {
    ClipCounts now;
    const int rc = clip_counts(ctx, opt.pairs, now);
    if (rc != PF_OK) return rc;
    r = clip_report_of(A, opt, now);
    return PF_OK;
}

}  // namespace pfh
