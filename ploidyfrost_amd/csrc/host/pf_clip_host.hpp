// `--adapters FILE [--adapter-seed S] [--adapter-score T]`: the host side of K-CLIP (pf_clip_begin .. pf_clip_end in ploidyfrost_hip.h, the
// rule in ../pf_clip_rule.hpp) for `trim`, `run` and `run-multi` -- the options, the adapter file read and refused before a device
// context exists, the clip opened on a context, and the line that reports it.
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
    bool on() const { return !adapters.empty(); }
};
struct ClipReport {   // what the `clip:` line says
    uint32_t adapters = 0, skipped = 0;
    pf_clip_stats stats = {};
};

// The file of opt.adapters read and parsed, seed and score checked: 0 = ok, else worded in err without the sub-command's name
// ("adapters <path>: record 3: an adapter holds 16 to 128 bases").  No device is touched.
inline int clip_load(const ClipOptions &opt, pf_clip::Adapters &A, std::string &err) {
    A.clear();
    { const int c = pf_clip::params_clause(opt.seed, opt.score); if (c) { err = pf_clip::refusal_text(c); return c; } }
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
    const int c = text.size() > (64u << 20) ? (int)pf_clip::REFUSE_NOT_FASTA : pf_clip::parse_adapters(text.data(), text.size(), A, &bad);
    if (c) { err = pf_clip::file_refusal(opt.adapters, c, bad); return c; }
    return 0;
}
// the clip opened on the context: PF_OK, or the ABI's code with pf_last_error
inline int clip_open(pf_ctx *ctx, const pf_clip::Adapters &A, const ClipOptions &opt) {
    return pf_clip_begin(ctx, A.bases.data(), A.off.data(), A.side.data(), A.size(), opt.seed, opt.score);
}
inline std::string clip_line(const ClipReport &r) {
    auto n = [](uint64_t v) { return std::to_string(v); };
    const pf_clip_stats &s = r.stats;
    return "clip: adapters " + n(r.adapters) + " skipped " + n(r.skipped) + " reads_clipped " + n(s.reads_clipped[0] + s.reads_clipped[1]) + " dropped " +
           n(s.reads_dropped[0] + s.reads_dropped[1]) + " bases_clipped " + n(s.bases_clipped[0] + s.bases_clipped[1]);
}
// the clip's statistics since its begin, less what `before` holds already, into the report
inline int clip_report(pf_ctx *ctx, const pf_clip::Adapters &A, const pf_clip_stats &before, ClipReport &r) {
    pf_clip_stats now = {};
    const int rc = pf_clip_stats_get(ctx, &now);
    if (rc != PF_OK) return rc;
    r.adapters = A.size();
    r.skipped = A.skipped;
    for (int f = 0; f < 2; ++f) {
        r.stats.reads_clipped[f] = now.reads_clipped[f] - before.reads_clipped[f];
        r.stats.reads_dropped[f] = now.reads_dropped[f] - before.reads_dropped[f];
        r.stats.bases_clipped[f] = now.bases_clipped[f] - before.bases_clipped[f];
        r.stats.candidates_scored[f] = now.candidates_scored[f] - before.candidates_scored[f];
    }
    return PF_OK;
}

}  // namespace pfh
