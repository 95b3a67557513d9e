// `ploidyfrost run`: steps 2 to 5 of the reference's workflow (script/pipeline/run.sh) for one sample in one process and on one device
// context -- what `mask -k ... --auto-cutoffs --db-out db`, `build -i -d -r filtered.fq` and the calling run `-g s.gfa -d db
// --auto-cutoffs` do with files between them:
//   count     the inputs through K-COUNT (count_stream), finished with the user's ci / cx / cs;
//   cut-offs  L and U from the histogram rows of the finished counters (counted_rows, cutoffs_from_rows), as --auto-cutoffs does;
//   table     pf_upload_counts: the table `mask` looks up and the calling run joins -- built once, resident to the end;
//   recount   the inputs a second time through K-MASKCOUNT (pf_maskcount_fastq, the rule in ../pf_run_rule.hpp): the k-mers of the
//             masked reads without the masked reads; finished with ci = 1;
//   graph     pf_unitig_build; its text stays on the device and goes to K-GFA through UnitigSet::open_gfa_memory;
//   calling   the CDBG constructor over the adopted context (CountsLoader::adopt), then the single-sample path exactly as the
//             command line sets it up (call_configure / call_run below, shared with pf_main.cpp).
// What is dead is freed before the next stage allocates: the first count's arrays after the upload (after --db-out has written
// them), the second count's after the graph is built, the device text after K-GFA has packed it.
#pragma once
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "pf_build_host.hpp"
#include "pf_cdbg.hpp"
#include "pf_count_host.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

// ---- the single-sample calling run behind a loaded CDBG, as the command line sets it up ----
struct CallSetup {
    std::string outprefix = "output";
    size_t threads = 1, ref_threads = 1;
    int lower = 10, upper = 1000;
    bool info = false, verbose = false;
    CDBG::ModelOptions model;               // --model ...
    const pf_filter_opts *filter = nullptr; // --filter "...": null = none
    unsigned density_points = 0;            // --density: 0 = off
    double density_adjust = 1.0;
};
// host threads, overlapped output, --ref-threads, the experiment switches of the environment.  0 = ok, else g.error()
int call_configure(CDBG &g, const CallSetup &s);
// model, filter and density settings, setUnitigId, printInfo, findSuperBubble, the two threshold lines, PloidyEstimation, the model's
// last line, with `verbose` the phase times -- on stdout, as `ploidyfrost -g -d` prints them.  mark (may be empty): called with the
// name of every finished phase.  0 = ok, else g.error()
int call_run(CDBG &g, const CallSetup &s, const std::function<void(const char *)> &mark = nullptr);

// ---- the coloured calling run behind a loaded CCDBG, as the command line sets it up (`ploidyfrost -g -f -d` and `run-multi`) ----
struct ColoredCallSetup {
    std::string outprefix = "output", graphfile;
    size_t threads = 1;
    bool info = false, verbose = false;
    CDBG::ModelOptions model;                            // --model ...
    const pf_filter_multi_opts *filter_multi = nullptr;  // --filter-multi "...": null = none
    bool each_color = false;                             // --model-each-color
    unsigned density_points = 0;                         // --density: 0 = off
    double density_adjust = 1.0;
    std::vector<std::pair<int, int>> cutoffs;            // one (lower, upper) per colour
    // --auto-cutoffs: the histogram rows of every colour's counters; the pairs are derived from them (max(10, cutoffL), cutoffU(q))
    const std::vector<std::vector<uint64_t>> *color_rows = nullptr;
    double quantile = 0.998;
};
// Thresholds per colour, host threads and overlapped output, model, filter-multi and density settings, setUnitigId, printInfo,
// findSuperBubble, the "Database i Minimum Coverage" lines, PloidyEstimation, the model's last line or the per-colour lines, with
// `verbose` the phase times -- on stdout / stderr, as `ploidyfrost -g -f -d` prints them.  s.cutoffs holds the pairs used afterwards.
// 0 = ok, else err holds the line for stderr.
int colored_call_run(CCDBG &g, ColoredCallSetup &s, std::string &err);

// ---- run ----
struct RunOptions {
    // the count (the workflow's defaults, not kmc's) and the graph (tips clipped, isolated unitigs removed)
    uint32_t k = 25;
    uint64_t ci = 1, cx = pf_count::DEFAULT_CX, cs = 10000;
    int g = BuildOptions::G_DEFAULT;
    bool clip_tips = true, del_isolated = true;
    uint64_t chunk_bytes = 0, initial_slots = 0;
    // thresholds: L = max(10, cutoffL), U = cutoffU(quantile) of the counted k-mers; mask_up bounds the masking as `mask -u` does
    double quantile = 0.998;
    uint32_t mask_up = 0xFFFFFFFFu;
    // the calling run
    size_t complex_size = 8;
    double match = 2, mismatch = -1, gap = -3;
    CallSetup call;   // (outprefix, lower and upper are filled in by run_fastq)
    // optional outputs, written through the writers of `mask --db-out` and `build`
    std::string db_out, gfa_out;
};
struct RunStats {
    pf_count_stats counted = {};       // the first pass, finished with ci / cx / cs
    uint32_t lower = 0, upper = 0;     // L, U
    pf_maskcount_stats masked = {};    // the second pass
    uint64_t distinct_kept = 0;        // distinct k-mers of the masked reads
    pf_unitig_stats graph = {};
    std::string model_last_line;       // with a model: what the calling run prints last
};
struct RunTimes {
    double count_s = 0, finish_s = 0, table_s = 0, db_out_s = 0, recount_s = 0, refinish_s = 0, graph_s = 0, gfa_out_s = 0, load_s = 0, call_s = 0;
};

// the refusal of the options that needs no file ("" = none): k outside 5 .. 31 (a database is implied), g, ci / cx / cs
std::string run_options_refusal(const RunOptions &opt);
// The whole of `ploidyfrost run`.  FASTA, gzip and an output that is an input are refused before a device context exists; L is
// printed on stdout as `mask --auto-cutoffs` prints it; --db-out and --gfa-out are written under temporary names and renamed at the
// end.  0 = ok, else worded in err (what the calling run itself refuses is worded as `ploidyfrost -g -d` words it).
int run_fastq(const std::vector<std::string> &inputs, const std::string &out_prefix, const RunOptions &opt, int device, RunStats &stats, RunTimes *times,
              std::string &err);

}  // namespace pfh
