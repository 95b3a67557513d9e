// `ploidyfrost smudge` and `run --smudge`: the host side of K-HETPAIR (pf_hetpairs in ploidyfrost_hip.h, the rule in
// ../pf_hetpair_rule.hpp) -- the Smudgeplot-style check of the ploidy estimate from the k-mer counts that are already on the device:
// a database decoded once (K-KMC) or the inputs counted (K-COUNT), the count table, the pairs, the report.  (The host's plain
// restatement of the rule, pf_hetpair::hetpairs_host, and the report text, pf_hetpair::report_text, live in the rule header itself.)
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../pf_hetpair_rule.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

struct CountOptions;   // pf_count_host.hpp

struct SmudgeOptions {
    uint32_t lo = 0, hi = 0;       // without auto_cutoffs
    bool auto_cutoffs = false;     // lo = what `cutoffL -d` prints, hi = what `cutoffU -d [quantile]` prints (K-HIST on the counters)
    double quantile = 0.998;
    uint64_t n = 0;                // haploid coverage; 0: no summary
    std::string pairs;             // --pairs FILE ("" = none)
};
struct SmudgeTimes {
    double load_s = 0;     // database: map, decode, histogram, table (with -k: the count of the inputs instead)
    double pairs_s = 0;    // pf_hetpairs
    double write_s = 0;    // the report and the pairs file
};
struct SmudgeResult {
    pf_hetpair_stats stats = {};
    uint32_t k = 0, lo = 0, hi = 0;   // the bounds that were used
    bool clamped = false;             // hi was lowered to lo + 4095
    pf_hetpair::Summary summary;      // with n
    SmudgeTimes times;
};

inline std::string smudge_report_path(const std::string &out) { return out + "_smudge.tsv"; }
// table, statistics and n to the report text
std::string smudge_report(const uint64_t *table, const pf_hetpair_stats &stats, uint32_t k, uint32_t lo, uint32_t hi, uint64_t n);
// The count table of `ctx` is resident and was uploaded from these device arrays: pf_hetpairs, the text of the report into `report`,
// and with pairs_fd >= 0 the lines of the pairs file written to it (pairs_name words a refusal).  `who` words the refusals ("smudge",
// "run").  0 = ok.  The caller opens, writes and renames the files.
int smudge_resident(pf_ctx *ctx, const char *who, const uint64_t *kmers_dev, const uint32_t *counts_dev, uint64_t n_keys, uint32_t k, uint32_t lo,
                    uint32_t hi, uint64_t n_hap, int pairs_fd, const std::string &pairs_name, SmudgeResult &res, std::string &report, std::string &err);
// `smudge -d db ... -o out`: what the sub-command does.  Refused before a device context exists: no output, the bounds
// (smudge_bounds_refusal), an output that is one of the database's files, a database counted with -b.  opt.n = 0: no summary (the
// command line and the Python wrapper refuse `-n` below 1).  0 = ok, else worded in err; nothing is left under any output name after a
// refusal
int smudge_db(const std::string &db_prefix, const SmudgeOptions &opt, const std::string &out, int device, SmudgeResult &res, std::string &err);
// `smudge -k ... -i reads -o out`: the inputs are counted first (count_stream, as `mask -k` uses it), then the same steps on the
// finished arrays -- what `count ... -o db` followed by `smudge -d db` gives
int smudge_counted(const CountOptions &count, const std::vector<std::string> &inputs, const SmudgeOptions &opt, const std::string &out, int device,
                   SmudgeResult &res, std::string &err);
// the bounds of the options as given (no auto_cutoffs): "" = fine, else the refusal's words
std::string smudge_bounds_refusal(const SmudgeOptions &opt);

}  // namespace pfh
