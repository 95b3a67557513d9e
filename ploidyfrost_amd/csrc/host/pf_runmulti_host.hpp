// `ploidyfrost run-multi`: the reference's multi-sample workflow (script/pipeline/run-multisample.sh) behind the trimmed reads in one
// process and on one device context -- what, for C samples, C times `mask -k ... --auto-cutoffs --db-out db<c> -o NAME_c`, one
// `build-multi -i -d -r NAME_0 -r NAME_1 ...` and the coloured calling run `-g s.gfa -f s.bfg_colors -d <list> --auto-cutoffs` do with
// C masked files, C databases, a graph and a colour file between them (the rule: ../pf_runmulti_rule.hpp):
//   first pass   per sample: its files through K-COUNT (count_stream), finished with the user's ci / cx / cs; L_c and U_c from the
//                histogram rows of the counters; the counter arrays stay resident: they are colour c of the joined table in the end;
//   second pass  per sample: pf_upload_counts of its arrays (it replaces the sample's before), its files through K-MASKCOUNT with
//                [L_c, -u], pf_count_finish(ci = 1): S_c, the sorted distinct k-mers of its masked reads;
//   union        K-UNION over S_0 .. S_{C-1}: the vertices, what `build-multi` counts from the masked files together;
//   graph        pf_unitig_build_colored, pf_color_begin(C);
//   colours      K-COLORSET: pf_color_kmers(c, S_c) per sample, each S_c freed behind it; pf_color_finish, pf_color_fetch,
//                pf_bfg::write into memory;
//   calling      the text stays on the device and goes to K-GFA (ColoredUnitigSet::open_memory), the colour sets are read from the
//                bytes in memory, the resident counters go to pf_upload_counts_colored (the adopting CCDBG constructor), then the
//                coloured calling run exactly as the command line sets it up (colored_call_run, shared with pf_main.cpp).
// What is dead is freed before the next stage allocates: a sample's table when the next sample's is uploaded (the last one's by
// pf_release_counts), S_c behind its colouring, the union behind pf_color_begin, the device text after K-GFA has packed it, the
// counters behind the joined table.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "pf_run_host.hpp"

namespace pfh {

struct MultiSample {
    std::string name;                  // the colour's name in the colour file
    std::vector<std::string> inputs;   // its FASTQ files
    bool paired = false;               // STEP... only: the inputs alternate file 1, file 2 (-1 / -2)
};
struct RunMultiOptions {
    RunOptions run;          // count, thresholds, graph, scoring, --db-out / --gfa-out prefixes (run.call is not used)
    ColoredCallSetup call;   // (outprefix, cutoffs and color_rows are filled in by run_multi_fastq)
    uint32_t n_seeds = 0;    // 0: pf_color::DEFAULT_SEEDS
};
struct RunMultiColor {
    uint32_t lower = 0, upper = 0;
    uint64_t distinct = 0, kept = 0;   // distinct k-mers counted; distinct k-mers of the masked reads
};
struct RunMultiStats {
    uint64_t colors = 0;
    uint64_t reads = 0, bases = 0, kmers = 0, bad = 0, distinct = 0;   // sums of the first passes
    uint64_t windows_bad = 0, windows_kept = 0;                        // sums of the second passes
    uint64_t distinct_kept = 0;                                        // the union: the vertices
    pf_unitig_stats graph = {};
    uint64_t kmers_colored = 0, kmers_unplaced = 0, runs = 0, overflow = 0, color_bytes = 0;
    std::vector<RunMultiColor> color;
    std::string model_last_line;
    std::vector<std::vector<ClipReport>> clip;      // --adapters: per sample the clipping of its first pass, one entry per unit
    std::vector<std::vector<pf_dedup_stats>> dedup; // --dedup: per sample the duplicates of its first pass, one entry per unit
    std::vector<std::vector<pf_trim_stats>> trim;   // STEP...: per sample the trimming of its first pass (paired: per input file, else one entry)
};
struct RunMultiTimes {
    double count_s = 0, db_out_s = 0, recount_s = 0, union_s = 0, graph_s = 0, color_s = 0, serialise_s = 0, gfa_out_s = 0, load_s = 0, call_s = 0;
};

// the refusals that need neither a file nor a device ("" = none): no sample, more than 1024, a sample without input, a name twice, a
// file in two samples by name
std::string run_multi_samples_refusal(const std::vector<MultiSample> &samples);
// The whole of `ploidyfrost run-multi`.  Everything above, FASTA, gzip (with opt.run.gz: gzip that is not blocked gzip), a file given twice under two names and an output that is an
// input are refused before a device context exists; every L_c is printed on its own line on stdout, in colour order; --db-out
// (<prefix><c>.kmc_pre / .kmc_suf) and --gfa-out (<prefix>.gfa, <prefix>.bfg_colors) are written under temporary names and renamed at
// the end.  0 = ok, else worded in err (what the calling run itself refuses is worded as `ploidyfrost -g -f -d` words it).
int run_multi_fastq(const std::vector<MultiSample> &samples, const std::string &out_prefix, const RunMultiOptions &opt, int device, RunMultiStats &stats,
                    RunMultiTimes *times, std::string &err);

}  // namespace pfh
