// `ploidyfrost build`: the host side of K-UNITIG (pf_unitig_* in ploidyfrost_hip.h, the rule in ../pf_unitig_rule.hpp) -- step
// `4.bifrost` of the reference's workflow (`Bifrost build -i -d -k 25 -r sample_filtered.fq -o sample`): the FASTQ inputs counted into
// the table in HBM as `count` does (every k-mer kept: ci = 1), the finished sorted k-mers compacted into unitigs on the device, the
// text of <out>.gfa downloaded in blocks.  (The host's plain restatement, pf_unitig::build_host, lives in the rule header itself.)
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../pf_color_rule.hpp"
#include "../pf_unitig_rule.hpp"
#include "pf_count_host.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

struct BuildOptions {   // Bifrost's letters
    static constexpr int G_DEFAULT = INT32_MIN;   // PFH_UNITIG_G_DEFAULT
    uint32_t k = 25;
    int g = G_DEFAULT;            // -g; G_DEFAULT: pf_unitig::default_g(k)
    bool clip_tips = false;       // -i
    bool del_isolated = false;    // -d
    uint64_t chunk_bytes = 0;     // 0: MASK_DEFAULT_CHUNK
    uint64_t initial_slots = 0;   // 0: twice the first chunk's bytes
    bool fasta = false;           // --fasta: inputs whose first byte is '>' are FASTA (K-FASTA, ../pf_fasta_rule.hpp)
};
struct BuildTimes {
    double stream_s = 0;   // first byte read to the last chunk counted (wall)
    double finish_s = 0;   // the count's flag, compact, sort
    double graph_s = 0;    // pf_unitig_build (wall); its stages on the device: pf_unitig_stats::stage_ms
    double write_s = 0;    // download and the file
};

// the refusal of the options ("" = none): k outside 3 .. 31, g outside 1 .. k - 2
std::string build_options_refusal(const BuildOptions &opt);
// The whole of `ploidyfrost build`: <out_prefix>.gfa, written under a temporary name and renamed at the end; nothing is left under
// either name after a refusal.  FASTA, gzip and an output that is an input are refused before a device context exists.  0 = ok, else
// worded in err (format refusals name the input and the 1-based record).
int build_fastq(const std::vector<std::string> &inputs, const std::string &out_prefix, const BuildOptions &opt, int device, pf_count_stats &counted,
                pf_unitig_stats &stats, BuildTimes *times, std::string &err);

// ---- `ploidyfrost build-multi`: the host side of K-COLOR (pf_color_* in ploidyfrost_hip.h, the rule in ../pf_color_rule.hpp) ----
struct ColoredTimes {
    BuildTimes build;
    double color_s = 0;       // every input streamed a second time (wall); its stages on the device: pf_color_stats
    double serialise_s = 0;   // runs and slots into the bytes of the colour file (host)
};
// the refusals of the inputs that need no file ("" = none): more than 1024, the same path twice
std::string colored_inputs_refusal(const std::vector<std::string> &inputs);
// The whole of `ploidyfrost build-multi`: <out_prefix>.gfa and <out_prefix>.bfg_colors, every input one colour in the order given,
// named by its path as given.  Both are written under temporary names and renamed at the end; nothing is left under any of the four
// names after a refusal.  n_seeds = 0: pf_color::DEFAULT_SEEDS.  0 = ok, else worded in err.
int build_colored_fastq(const std::vector<std::string> &inputs, const std::string &out_prefix, const BuildOptions &opt, uint32_t n_seeds, int device,
                        pf_count_stats &counted, pf_unitig_stats &stats, pf_color_stats &colored, uint64_t &color_bytes, ColoredTimes *times,
                        std::string &err);

}  // namespace pfh
