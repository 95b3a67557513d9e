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
#include "pf_clip_host.hpp"
#include "pf_dedup_host.hpp"
#include "pf_qc_host.hpp"
#include "pf_hetpair_host.hpp"
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

// ---- `run STEP...` / `run-multi STEP...`: step 1 of the workflow folded in (K-TRIMCOUNT, the rule in ../pf_trimrun_rule.hpp) ----
// The inputs are the raw reads; both passes stream them and trim again through pf_count_fastq[_pair]_trimmed and
// pf_maskcount_fastq[_pair]_trimmed.  Nothing per record is kept between the passes, so the result does not depend on the chunking.
struct TrimInputs {
    std::vector<pf_trim_step> steps;   // none: no trimming, the inputs are read as they are
    uint32_t phred = 33;
    ClipOptions clip;                  // --adapters: K-CLIP in front of the steps; turns trimming on as a step does
    DedupOptions dedup;                // --dedup: K-DEDUP behind the steps, a fresh table per unit in both passes; turns trimming on as a step does
    bool on() const { return !steps.empty() || clip.on() || dedup.on; }
};
// A unit is what one `trim` command of the equivalent chain takes: all single-ended files together, or one pair.
inline size_t trim_unit_count(size_t n_inputs, bool paired) { return paired ? n_inputs / 2 : 1; }
// what is refused about the inputs of a trimmed run before a device context exists ("" = none), without the sub-command's name:
// a pair without its second file, steps or phred K-TRIM refuses, a file given twice (by name or as one file under two names)
std::string trim_inputs_refusal(const std::vector<std::string> &inputs, bool paired, const TrimInputs &trim);
// One pass over the raw reads into the open count: masked = false through pf_count_fastq[_pair]_trimmed, true through
// pf_maskcount_fastq[_pair]_trimmed with [low, up].  paired: the inputs alternate file 1, file 2, and every pair goes through the
// lock-step stream of pf_reads_stream.hpp; else they go through stream_fastq one after the other.  The inputs are what the preflight
// made of them, the same for both passes.  unit_stats (may be null; paired: one entry per input file, else one entry) and masked_stats
// (may be null) are added to.  unit_clip (may be null; a clip is open on the context): one entry per unit, what the clip counted
// while the unit streamed.  With trim.dedup a fresh dedup is opened for every unit and closed behind it; unit_dedup (may be null): one
// entry per unit, its statistics.  0 = ok, else worded in err by `who`.
int stream_trimmed(pf_ctx *ctx, const char *who, const std::vector<ReadsInput> &inputs, bool paired, const TrimInputs &trim, uint64_t chunk_bytes,
                   bool masked, uint32_t low, uint32_t up, pf_trim_stats *unit_stats, pf_maskcount_stats *masked_stats, std::string &err,
                   ClipCounts *unit_clip = nullptr, pf_dedup_stats *unit_dedup = nullptr);
// the `trim:` line of a unit on stderr, in `trim`'s own format: st = the unit's statistics (paired: of file 1 and of file 2)
std::string trim_unit_line(const pf_trim_stats *st, bool paired);

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
    // STEP...: the inputs are raw reads (paired: -1 / -2, alternating file 1, file 2)
    TrimInputs trim;
    bool paired = false;
    int gz = 0;        // --gz (1), --gz-plain (2: any gzip, K-GUNZIP): inputs with the gzip magic are blocked gzip, inflated on the device in both passes (pf_gz_host.hpp)
    std::string report;   // --report (with opt.trim alone): K-QC's report of both stages over the first pass, the one `trim --report` writes for the same inputs
    bool fasta = false;   // --fasta: a chunk whose first byte is '>' goes through pf_count_fasta / pf_maskcount_fasta in the two passes (K-FASTA); not with trim steps
    // --smudge [--smudge-n N] [--smudge-pairs FILE]: K-HETPAIR behind the table of the first pass (pf_hetpair_host.hpp), lo = L,
    // hi = min(U, L + 4095); PloidyFrost_output/<o>_smudge.tsv beside the calling run's files
    bool smudge = false;
    uint64_t smudge_n = 0;
    bool smudge_n_seen = false;
    std::string smudge_pairs;
};
struct RunStats {
    pf_count_stats counted = {};       // the first pass, finished with ci / cx / cs
    uint32_t lower = 0, upper = 0;     // L, U
    pf_maskcount_stats masked = {};    // the second pass
    uint64_t distinct_kept = 0;        // distinct k-mers of the masked reads
    pf_unitig_stats graph = {};
    std::string model_last_line;       // with a model: what the calling run prints last
    std::vector<pf_trim_stats> trim;   // STEP...: the trimming of the first pass (paired: one entry per input file, else one entry)
    std::vector<ClipReport> clip;      // --adapters: the clipping of the first pass, one entry per unit
    std::vector<pf_dedup_stats> dedup; // --dedup: the duplicates of the first pass, one entry per unit
    QcReport qc;                       // --report: the tables of the first pass
    SmudgeResult smudge;               // --smudge
};
struct RunTimes {
    double count_s = 0, finish_s = 0, table_s = 0, db_out_s = 0, recount_s = 0, refinish_s = 0, graph_s = 0, gfa_out_s = 0, load_s = 0, call_s = 0;
    double smudge_s = 0;   // --smudge: K-HETPAIR and the report's text
};

// the refusal of the options that needs no file ("" = none): k outside 5 .. 31 (a database is implied), g, ci / cx / cs
std::string run_options_refusal(const RunOptions &opt);
// The whole of `ploidyfrost run`.  FASTA, gzip (with opt.gz: gzip that is not blocked gzip) and an output that is an input are refused before a device context exists; L is
// printed on stdout as `mask --auto-cutoffs` prints it; --db-out and --gfa-out are written under temporary names and renamed at the
// end.  With opt.trim.steps the inputs are the raw reads and every file `run` writes is what `trim` followed by `run` on the trimmed
// reads of the pairs kept whole (o1 / o2; single-ended: -o) writes.  0 = ok, else worded in err (what the calling run itself refuses
// is worded as `ploidyfrost -g -d` words it).
int run_fastq(const std::vector<std::string> &inputs, const std::string &out_prefix, const RunOptions &opt, int device, RunStats &stats, RunTimes *times,
              std::string &err);

}  // namespace pfh
