// `ploidyfrost build` and `ploidyfrost build-multi`: one command line, the graph of the reads and, coloured, the colour file beside it
#include <algorithm>
#include <iostream>
#include <string>
#include <vector>

#include "pf_build_host.hpp"
#include "pf_cli.hpp"
#include "pf_cli_subs.hpp"

using namespace std;
using namespace pfcli;

// `build`: step `4.bifrost` of the reference's workflow (`Bifrost build -i -d -k 25 -r sample_filtered.fq -o sample`) on the device.  The
// letters are Bifrost's: -i clips tips here, the reads come with -r.
// `build-multi`: the last step of the reference's multi-sample workflow (`Bifrost build -i -d -k 25 -r s0.fq -r s1.fq ... -c -o sample`)
// on the device: the graph of `build` from all files together, and the colour file with one colour per -r in the order given.
int build_main(int argc, char **argv, bool colored) {
    static const struct { const char *sub, *usage, *all_there_is; } kinds[2] = {
        {"build", "Usage:PloidyFrost build -k 25 [-i] [-d] -r reads.fq [-r more.fq ...] -o sample [-g G] [-t N] [--chunk-bytes N] [--initial-slots N] [--fasta] [-v]",
         "a single-sample graph of the reads given with -r, written as GFA, is all there is"},
        {"build-multi", "Usage:PloidyFrost build-multi -k 25 [-i] [-d] -r s0.fq -r s1.fq [-r ...] -o sample [-g G] [-t N] [--chunk-bytes N] [--initial-slots N] [--fasta] [-v]",
         "the coloured graph of the reads given with -r, one colour a file, is all there is"},
    };
    const auto &kind = kinds[colored];
    const Refuse refuse{kind.sub, kind.usage};
    pfh::BuildOptions opt;
    string out;
    vector<string> inputs;
    ReadsCli reads(ReadsCli::FASTA | ReadsCli::CHUNK | ReadsCli::SLOTS);
    static const char *const not_built[] = {"-s", "-c", "-y", "-f", "-a", "-m", "-n", "-b", "-B", "-l", "-w", "-e"};
    for (int i = 2; i < argc; ++i) {
        const string a = argv[i];
        string why;
        if (colored && a == "-c") continue;   // (Bifrost's letter for what build-multi always does)
        for (const char *nb : not_built)
            if (a == nb) return refuse(a + " is not built (" + kind.all_there_is + ")" + (a == "-c" ? "; the coloured graph of several samples: `build-multi`" : ""));
        if (a == "--gpus") return refuse("--gpus is not built: the graph is made on one GPU");
        if (a == "-i") { opt.clip_tips = true; continue; }
        if (a == "-d") { opt.del_isolated = true; continue; }
        if (const int taken = reads.take(argc, argv, i, why)) { if (taken < 0) return refuse(why); continue; }
        if (a != "-k" && a != "-g" && a != "-t" && a != "-r" && a != "-o") return refuse("unknown option " + a);
        const char *val = value_of(argc, argv, i, why);
        uint64_t v = 0;
        if (!val) return refuse(why);
        if (a == "-r") inputs.push_back(val);
        else if (a == "-o") out = val;
        else if (!number(a, val, v, true, why)) return refuse(why);
        else if (a == "-k") opt.k = (uint32_t)std::min<uint64_t>(v, 0xFFFFFFFFull);
        else if (a == "-g") opt.g = (int)std::min<uint64_t>(v, 0x7FFFFFFFull);
        // (-t: accepted and ignored)
    }
    opt.fasta = reads.fasta;
    opt.chunk_bytes = reads.chunk_bytes;
    opt.initial_slots = reads.initial_slots;
    // refused by name, before anything is read or written
    if (inputs.empty()) return refuse("-r <reads.fq> is missing");
    if (out.empty()) return refuse("-o <sample> is missing");
    { const string why = pfh::build_options_refusal(opt); if (!why.empty()) return refuse(why); }
    if (colored) { const string why = pfh::colored_inputs_refusal(inputs); if (!why.empty()) return refuse(why); }
    pf_count_stats cst = {};
    pf_unitig_stats st = {};
    pf_color_stats col = {};
    uint64_t color_bytes = 0;
    pfh::ColoredTimes tm;
    string err;
    if (colored ? pfh::build_colored_fastq(inputs, out, opt, 0, 0, cst, st, col, color_bytes, &tm, err) : pfh::build_fastq(inputs, out, opt, 0, cst, st, &tm.build, err)) return failed(err);
    if (colored) {
        cerr << "build-multi: colors " << col.colors << " reads " << cst.reads << " bases " << cst.bases << " kmers " << cst.kmers << " bad " << cst.kmers_bad
             << " distinct " << st.distinct << " unitigs " << st.unitigs << " removed " << st.removed << " unitigs_out " << st.unitigs_out << " longest "
             << st.longest << " bytes " << st.bytes << " windows_colored " << col.windows_colored << " windows_unplaced " << col.windows_unplaced << " runs "
             << col.runs << " overflow " << col.overflow << " color_bytes " << color_bytes << endl;
        if (reads.verbose) {
            cerr << "build-multi: stream " << tm.build.stream_s << "s finish " << tm.build.finish_s << "s graph " << tm.build.graph_s << "s color " << tm.color_s
                 << "s serialise " << tm.serialise_s << "s write " << tm.build.write_s << "s; device ms: index " << st.stage_ms[0] << " adjacency " << st.stage_ms[1]
                 << " simplify " << st.stage_ms[2] << " rank " << st.stage_ms[3] << " cycles " << st.stage_ms[4] << " emit " << st.stage_ms[5] << " table "
                 << col.table_ms << " mark " << col.mark_ms << " runs " << col.runs_ms << endl;
        }
        return 0;
    }
    cerr << "build: reads " << cst.reads << " bases " << cst.bases << " kmers " << cst.kmers << " bad " << cst.kmers_bad << " distinct " << st.distinct
         << " unitigs " << st.unitigs << " removed " << st.removed << " unitigs_out " << st.unitigs_out << " longest " << st.longest << " bytes " << st.bytes
         << (st.distinct == 0 ? " (no k-mer in the input: the header line alone is written)" : "") << endl;
    if (reads.verbose) {
        cerr << "build: stream " << tm.build.stream_s << "s finish " << tm.build.finish_s << "s graph " << tm.build.graph_s << "s write " << tm.build.write_s
             << "s; device ms: index " << st.stage_ms[0] << " adjacency " << st.stage_ms[1] << " simplify " << st.stage_ms[2] << " rank " << st.stage_ms[3] << " ("
             << st.rounds << " rounds) cycles " << st.stage_ms[4] << " (" << st.cycles << " closed, " << st.cycle_rounds << " rounds) emit " << st.stage_ms[5] << endl;
    }
    return 0;
}
