// `ploidyfrost qc` and `--report FILE` of `trim` / `run`: the host side of K-QC (pf_qc_begin .. pf_qc_end in ploidyfrost_hip.h, the rule
// and the text of the report in ../pf_qc_rule.hpp) -- the report opened on a context, its tables fetched and worded, and the stream
// of `qc` itself.  The report is a function of the tables alone; the device adds to them, the host never looks at a read.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../pf_qc_rule.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

struct QcReport {   // what a report held when it was closed
    uint32_t phred = 33;
    std::vector<uint64_t> tables;   // [side][stage][pf_qc::TABLE_WORDS]
    std::vector<uint64_t> clip;     // [side][pf_qc::CLIP_WORDS]; empty: no clip was open
    std::string text() const { return pf_qc::report_text(tables.data(), clip.empty() ? nullptr : clip.data(), phred); }
    // the lines for stderr: one per side that was seen, then the warning about the quality offset where there is one
    std::vector<std::string> lines() const {
        std::vector<std::string> o;
        if (tables.empty()) return o;
        for (uint32_t side = 0; side < 2; ++side) {
            const uint64_t *raw = tables.data() + (size_t)(side * pf_qc::STAGES + pf_qc::STAGE_RAW) * pf_qc::TABLE_WORDS;
            if (raw[pf_qc::W_SEEN]) o.push_back(pf_qc::side_line(side, raw));
        }
        const std::string warn = pf_qc::hint_line(tables.data(), phred);
        if (!warn.empty()) o.push_back(warn);
        return o;
    }
};

// the report opened on the context: 0 = ok, else worded in err by `who`
inline int qc_open(pf_ctx *ctx, uint32_t phred, const char *who, std::string &err) {
    if (pf_qc_begin(ctx, phred) == PF_OK) return 0;
    err = std::string(who) + ": " + pf_last_error(ctx);
    return 1;
}
// the tables of the open report into r, and the report closed (clip_open: the clip curves are part of it)
inline int qc_close(pf_ctx *ctx, uint32_t phred, bool clip_open, const char *who, QcReport &r, std::string &err) {
    r = QcReport{};
    r.phred = phred;
    r.tables.assign((size_t)2 * pf_qc::STAGES * pf_qc::TABLE_WORDS, 0);
    if (clip_open) r.clip.assign((size_t)2 * pf_qc::CLIP_WORDS, 0);
    int rc = PF_OK;
    for (int side = 0; side < 2 && rc == PF_OK; ++side) {
        for (int stage = 0; stage < (int)pf_qc::STAGES && rc == PF_OK; ++stage)
            rc = pf_qc_get(ctx, side, stage, r.tables.data() + (size_t)(side * pf_qc::STAGES + stage) * pf_qc::TABLE_WORDS);
        if (rc == PF_OK && clip_open) rc = pf_qc_clip_get(ctx, side, r.clip.data() + (size_t)side * pf_qc::CLIP_WORDS);
    }
    if (rc == PF_OK) rc = pf_qc_end(ctx);
    if (rc == PF_OK) return 0;
    err = std::string(who) + ": " + pf_last_error(ctx);
    return 1;
}

struct QcOptions {
    uint32_t phred = 33;
    int gz = 0;                 // --gz (1), --gz-plain (2), as `count` takes them
    uint64_t chunk_bytes = 0;   // 0 = MASK_DEFAULT_CHUNK (pf_reads_stream.hpp)
};
// `ploidyfrost qc`: every file streamed on its own through pf_qc_fastq, inputs1 to side 1 and inputs2 to side 2 (stage raw alone; the
// sides are not held to equal record counts).  The report is written under a temporary name and renamed at the end; nothing is left
// under its name after a refusal.  What needs no device -- no input, no report path, a quality offset other than 33 or 64, the gzip
// and format refusals of `count`, a report path that is an input -- is refused before a device context exists.  0 = ok, else worded
// in err.
int qc_fastq(const std::vector<std::string> &inputs1, const std::vector<std::string> &inputs2, const std::string &report_path, const QcOptions &opt,
             int device, QcReport &report, std::string &err);

}  // namespace pfh
