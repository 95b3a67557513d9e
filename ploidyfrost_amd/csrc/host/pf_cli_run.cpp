// `ploidyfrost run` and `ploidyfrost run-multi`: reads to ploidy estimate in one process.  What the two command lines share is RunCli;
// each keeps the options it refuses by name, the rules of its inputs and its summary lines.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "pf_cli.hpp"
#include "pf_cli_subs.hpp"
#include "pf_hetpair_host.hpp"
#include "pf_run_host.hpp"
#include "pf_runmulti_host.hpp"

using namespace std;
using namespace pfcli;

namespace {
// the letters of `count` / `mask` (-k -ci -cs -cx -u), of `trim` (STEP... --phred --adapters ... -1 -2), of `build` (-g), of the calling
// run (-z -M -D -G -t -q, and its long options --model ... --filter ... --density ...) and the reads options
struct RunCli {
    const char *sub;
    pfh::RunOptions &opt;
    Options lopt;   // the long options of the calling run
    DensityCli dc;
    CountArgs c;
    TrimCli tc;
    ReadsCli reads{ReadsCli::ALL};
    string out;
    size_t threads = 1;
    pf_filter_opts filter = {};
    pf_filter_multi_opts multi = {};

    RunCli(const char *sub_, pfh::RunOptions &opt_) : sub(sub_), opt(opt_) {
        c.opt.ci = opt.ci;
        c.opt.cx = opt.cx;
        c.opt.cs = opt.cs;
    }
    // a word that both sub-commands take; the files of -1 / -2 go to `files`
    int take(int argc, char **argv, int &i, vector<string> &files, string &why) {
        const string a = argv[i];
        if (const int taken = c.take(argc, argv, i, why)) return taken;
        if (const int taken = tc.take(argc, argv, i, sub, files, why)) return taken;
        if (const int taken = reads.take(argc, argv, i, why)) return taken;
        if (a == "--keep-tips") { opt.clip_tips = false; return 1; }
        if (a == "--keep-isolated") { opt.del_isolated = false; return 1; }
        if (a != "-o" && a != "-q" && a != "-u" && a != "-g" && a != "-z" && a != "-M" && a != "-D" && a != "-G" && a != "-t" && a != "--db-out" && a != "--gfa-out") return 0;
        const char *val = value_of(argc, argv, i, why);
        if (!val) return -1;
        uint64_t v = 0;
        if (a == "-o") out = val;
        else if (a == "--db-out") opt.db_out = val;
        else if (a == "--gfa-out") opt.gfa_out = val;
        else if (a == "-q" || a == "-M" || a == "-D" || a == "-G") return real(a, val, a == "-q" ? opt.quantile : a == "-M" ? opt.match : a == "-D" ? opt.mismatch : opt.gap, why) ? 1 : -1;
        else if (a == "-u") {
            if (!number(a, val, v, false, why)) return -1;
            if (v > 0xFFFFFFFFull) { why = string("-u takes a number from 0 to 4294967295, not '") + val + "'"; return -1; }
            opt.mask_up = (uint32_t)v;
        }
        else if (!number(a, val, v, true, why)) return -1;
        else if (a == "-g") opt.g = (int)std::min<uint64_t>(v, 0x7FFFFFFFull);
        else if (a == "-z") opt.complex_size = (size_t)v;
        else threads = (size_t)v;
        return 1;
    }
    // behind the last word, in front of the sub-command's rules for its inputs: the trim words ("" = accepted)
    string finish_trim() {
        opt.trim.phred = tc.phred.phred;
        return tc.finish(sub, opt.trim.steps, opt.trim.clip, opt.trim.dedup);
    }
    // behind those rules: the fields of the count and of the reads, what the host layer refuses, the range checks of the calling run
    string finish() {
        opt.k = c.opt.k;
        opt.ci = c.opt.ci;
        opt.cx = c.opt.cx;
        opt.cs = c.opt.cs;
        opt.gz = reads.gz;
        opt.fasta = reads.fasta;
        opt.chunk_bytes = reads.chunk_bytes;
        opt.initial_slots = reads.initial_slots;
        { const string why = pfh::run_options_refusal(opt); if (!why.empty()) return why; }
        if (opt.quantile < 0 || opt.quantile > 1) return "-q: frequency cutoff value should be between 0 and 1";
        if (opt.complex_size < 4) return "-z: Maximum number of unitigs in superbubble is at least 4 !";
        if (opt.mismatch > opt.match) return "-D: Mismatch penalty should be smaller than match score !";
        if (opt.gap > opt.match) return "-G: Gap penalty should be smaller than match score !";
        if (threads > std::thread::hardware_concurrency()) return "-t: Number of threads cannot be greater than " + to_string(std::thread::hardware_concurrency());
        return "";
    }
    // --model / --filter / --filter-multi / --density into the set-up of the calling run; false: refused, model_setup has said why
    template <class Call> bool hand_off(Call &call) {
        if (!model_setup(lopt, dc, call.model, filter, multi)) return false;
        call.threads = threads;
        call.verbose = reads.verbose;
        call.density_points = dc.on ? dc.points : 0;
        call.density_adjust = dc.adjust;
        return true;
    }
    // the chain failed: what its last command says on stdout is said there; its own refusals carry their "Error:" already
    int failed(const string &err, const char *graph_read) const {
        cout.flush();
        fflush(nullptr);
        if (err.rfind(graph_read, 0) == 0) cout << err << endl;
        else if (err.rfind(string(sub) + ": ", 0) == 0) cerr << "Error: " << err << endl;
        else cerr << err << endl;
        return EXIT_FAILURE;
    }
};
}  // namespace

// `run`: steps 2 to 5 of the reference's workflow for one sample (`kmc`, `kmc_tools filter`, `Bifrost build`, `PloidyFrost`) in one
// process and on one device context
int run_main(int argc, char **argv) {
    const Refuse refuse{"run", "Usage:PloidyFrost run [-k 25] [-ci 1] [-cs 10000] [-cx N] -i trimmed.fq [-i more.fq ...] -o sample [-q Q] [-u U] [--keep-tips] [--keep-isolated] [-g G]\n"
                               "                 [-z Z -M m -D d -G g -t T --ref-threads N] [--model cov|fre ... --model-only --filter \"OPTS\" --density ...]\n"
                               "                 [--db-out <KMCDatabase>] [--gfa-out <sample>] [--chunk-bytes N] [--initial-slots N] [--gz] [--gz-plain] [--fasta] [-v]\n"
                               "      PloidyFrost run [the same options] -i raw.fq [-i more.fq ...] -o sample STEP... [--phred 33|64]\n"
                               "      PloidyFrost run [the same options] -1 r1.fq -2 r2.fq [-1 r3.fq -2 r4.fq ...] -o sample STEP... [--phred 33|64]\n"
                               "      STEP: LEADING:t TRAILING:t SLIDINGWINDOW:w:t MINLEN:l (the raw reads are trimmed on the way in, as `trim` trims them)\n"
                               "      [--report report.tsv] with STEP... or --adapters: the read quality report `trim --report` writes for the same inputs\n"
                               "      [--smudge [--smudge-n N] [--smudge-pairs FILE]]: the k-mer pair report `smudge` writes for the counted k-mers, as PloidyFrost_output/<sample>_smudge.tsv"};
    pfh::RunOptions opt;
    RunCli cli("run", opt);
    const Options &lopt = cli.lopt;
    if (!take_long_options(argc, argv, 2, cli.lopt, cli.dc)) return 1;
    vector<string> inputs, pair_files;
    static const struct { const char *name, *why; } not_here[] = {
        {"-f", "-f is not built into run: the coloured workflow goes in steps (`build-multi`, then the calling run with -f)"},
        {"-C", "-C does not go with run: the thresholds come from the counted k-mers (one sample, no coverage file)"},
        {"-d", "-d does not go with run: the database is counted from the reads (--db-out writes it; isolated unitigs are removed unless --keep-isolated)"},
        {"-h", "-h does not go with run: the thresholds come from the counted k-mers, not from a histogram file"},
        {"-l", "-l does not go with run: the lower threshold is derived from the counted k-mers (as --auto-cutoffs derives it)"},
        {"-b", "-b does not go with run: the graph is built from both strands"},
        {"--filtered-out", "--filtered-out is not built: the masked reads are never made (`mask` writes them)"},
        {"--detach-teardown", "--detach-teardown is not built into run"},
    };
    if (lopt.gpus_seen) return refuse("--gpus is not built into run: one sample, one GPU");
    if (lopt.each_color || lopt.multi_seen) return refuse("--filter-multi / --model-each-color belong to the coloured path: run has --filter");
    if (lopt.detach_teardown) return refuse(not_here[7].why);
    for (int i = 2; i < argc; ++i) {
        const string a = argv[i];
        string why;
        for (const auto &nh : not_here)
            if (a == nh.name) return refuse(nh.why);
        if (const int taken = cli.take(argc, argv, i, pair_files, why)) { if (taken < 0) return refuse(why); continue; }
        if (a == "--smudge") { opt.smudge = true; continue; }
        if (a != "-i" && a != "--report" && a != "--smudge-n" && a != "--smudge-pairs") return refuse("unknown option " + a);
        const char *val = value_of(argc, argv, i, why);
        if (!val) return refuse(why);
        if (a == "-i") inputs.push_back(val);
        else if (a == "--smudge-n") { if (!number(a, val, opt.smudge_n, false, why)) return refuse(why); opt.smudge_n_seen = true; }
        else if (!*val) return refuse(a + " needs a value");
        else (a == "--report" ? opt.report : opt.smudge_pairs) = val;
    }
    // refused by name, before anything is read or written and before a device context exists
    { const string why = cli.finish_trim(); if (!why.empty()) return refuse(why); }
    if (cli.tc.pair_seen && !inputs.empty()) return refuse("-i does not go with -1 / -2 (the inputs are either single-ended or pairs)");
    if (cli.tc.pair_seen) { inputs = pair_files; opt.paired = true; }
    if (inputs.empty()) return refuse("-i <reads.fq> is missing");
    if (cli.out.empty()) return refuse("-o <sample> is missing");
    { const string why = cli.finish(); if (!why.empty()) return refuse(why); }
    pf_filter_opts &filter = cli.filter;
    if (!cli.hand_off(opt.call)) return 1;
    opt.call.ref_threads = lopt.ref_threads;
    opt.call.filter = lopt.filter_seen ? &filter : nullptr;
    const bool verbose = cli.reads.verbose;
    pfh::RunStats st;
    pfh::RunTimes tm;
    string err;
    if (pfh::run_fastq(inputs, cli.out, opt, 0, st, &tm, err)) return cli.failed(err, "CompactedDBG::read()");
    for (size_t u = 0; u < pfh::trim_unit_count(inputs.size(), opt.paired) && opt.trim.on(); ++u) {   // one line per `trim` of the equivalent chain
        if (u < st.clip.size()) cerr << pfh::clip_line(st.clip[u]) << endl;
        if (u < st.dedup.size()) cerr << pfh::dedup_line(st.dedup[u]) << endl;
        cerr << pfh::trim_unit_line(&st.trim[opt.paired ? 2 * u : 0], opt.paired) << endl;
    }
    for (const string &l : st.qc.lines()) cerr << l << endl;
    cerr << "run: reads " << st.counted.reads << " bases " << st.counted.bases << " kmers " << st.counted.kmers << " bad " << st.counted.kmers_bad << " distinct "
         << st.counted.unique << " lower " << st.lower << " upper " << st.upper << " windows_bad " << st.masked.kmers_bad << " windows_kept " << st.masked.kmers_kept
         << " distinct_kept " << st.distinct_kept << " unitigs " << st.graph.unitigs << " removed " << st.graph.removed << " unitigs_out " << st.graph.unitigs_out
         << " longest " << st.graph.longest << endl;
    if (opt.smudge) {
        pf_hetpair::Stats hs;
        hs.kmers = st.smudge.stats.kmers; hs.in_range = st.smudge.stats.in_range; hs.one_partner = st.smudge.stats.one_partner;
        hs.many_partners = st.smudge.stats.many_partners; hs.pairs = st.smudge.stats.pairs;
        cerr << pf_hetpair::stats_text(hs) << endl;
        if (opt.smudge_n) cerr << pf_hetpair::proposed_text(st.smudge.summary) << endl;
        if (verbose) cerr << "smudge: pairs " << st.smudge.times.pairs_s << "s (inside run: " << tm.smudge_s << "s)" << endl;
    }
    if (verbose)
        cerr << "run: count " << tm.count_s << "s finish " << tm.finish_s << "s table " << tm.table_s << "s db-out " << tm.db_out_s << "s recount " << tm.recount_s
             << "s refinish " << tm.refinish_s << "s graph " << tm.graph_s << "s gfa-out " << tm.gfa_out_s << "s load " << tm.load_s << "s call " << tm.call_s << "s" << endl;
    return 0;
}

// `run-multi`: the multi-sample workflow (script/pipeline/run-multisample.sh) behind the trimmed reads in one process and on one device
// context; `run`'s letters, with --sample NAME in front of every sample's -i and the coloured run's --filter-multi / --model-each-color
int run_multi_main(int argc, char **argv) {
    const Refuse refuse{"run-multi", "Usage:PloidyFrost run-multi [-k 25] [-ci 1] [-cs 10000] [-cx N] --sample NAME -i a.fq [-i b.fq ...] --sample NAME2 -i c.fq [...] -o out\n"
                                     "                 [-q Q] [-u U] [--keep-tips] [--keep-isolated] [-g G] [-z Z -M m -D d -G g -t T --ref-threads N]\n"
                                     "                 [--model cov|fre --filter-multi \"OPTS\" [--model-each-color] [--density ...] [--model-only]]\n"
                                     "                 [--db-out <KMCDatabase>] [--gfa-out <graph>] [--chunk-bytes N] [--initial-slots N] [--gz] [--gz-plain] [--fasta] [-v]\n"
                                     "      PloidyFrost run-multi [the same options] --sample NAME (-i raw.fq ... | -1 r1.fq -2 r2.fq ...) --sample NAME2 ... -o out STEP... [--phred 33|64]\n"
                                     "      STEP: LEADING:t TRAILING:t SLIDINGWINDOW:w:t MINLEN:l (the raw reads are trimmed on the way in, as `trim` trims them)"};
    pfh::RunMultiOptions mopt;
    RunCli cli("run-multi", mopt.run);
    Options &lopt = cli.lopt;
    if (!take_long_options(argc, argv, 2, lopt, cli.dc)) return 1;
    vector<pfh::MultiSample> samples;
    static const struct { const char *name, *why; } not_here[] = {
        {"-f", "-f does not go with run-multi: the colour file is made from the samples (--gfa-out writes it)"},
        {"-C", "-C does not go with run-multi: the thresholds come from every sample's counted k-mers (no coverage file)"},
        {"-d", "-d does not go with run-multi: the databases are counted from the reads (--db-out writes them; isolated unitigs are removed unless --keep-isolated)"},
        {"-h", "-h does not go with run-multi: the thresholds come from every sample's counted k-mers, not from histogram files"},
        {"-l", "-l does not go with run-multi: the lower thresholds are derived from the counted k-mers (as --auto-cutoffs derives them)"},
        {"-b", "-b does not go with run-multi: the graph is built from both strands"},
        {"--filtered-out", "--filtered-out is not built: the masked reads are never made (`mask` writes them)"},
        {"--detach-teardown", "--detach-teardown is not built into run-multi"},
    };
    if (lopt.gpus_seen) return refuse("--gpus is not built into run-multi: the coloured path runs on one GPU");
    if (lopt.filter_seen) return refuse("--filter reads the single-sample result streams: run-multi has --filter-multi");
    if (lopt.detach_teardown) return refuse(not_here[7].why);
    for (int i = 2; i < argc; ++i) {
        const string a = argv[i];
        string why;
        for (const auto &nh : not_here)
            if (a == nh.name) return refuse(nh.why);
        const bool pair_file = a == "-1" || a == "-2";
        if (pair_file && samples.empty()) return refuse(a + " stands before any --sample NAME: every input belongs to a sample");
        if (pair_file && !samples.back().paired && !samples.back().inputs.empty())
            return refuse("sample " + samples.back().name + ": -i does not go with -1 / -2 (the inputs of a sample are either single-ended or pairs)");
        if (a == "--sample" && !cli.tc.pending1.empty()) return refuse(cli.tc.no_second());
        static vector<string> no_files;
        if (const int taken = cli.take(argc, argv, i, samples.empty() ? no_files : samples.back().inputs, why)) {
            if (taken < 0) return refuse(why);
            if (pair_file) samples.back().paired = true;
            continue;
        }
        if (a != "--sample" && a != "-i") return refuse("unknown option " + a);
        const char *val = value_of(argc, argv, i, why);
        if (!val) return refuse(why);
        if (a == "--sample") { samples.emplace_back(); samples.back().name = val; }
        else {
            if (samples.empty()) return refuse(string("-i ") + val + " stands before any --sample NAME: every input belongs to a sample");
            if (samples.back().paired) return refuse("sample " + samples.back().name + ": -i does not go with -1 / -2 (the inputs of a sample are either single-ended or pairs)");
            samples.back().inputs.push_back(val);
        }
    }
    // refused by name, before anything is read or written and before a device context exists
    { const string why = cli.finish_trim(); if (!why.empty()) return refuse(why); }
    { const string why = pfh::run_multi_samples_refusal(samples); if (!why.empty()) return refuse(why); }
    if (cli.out.empty()) return refuse("-o <out> is missing");
    { const string why = cli.finish(); if (!why.empty()) return refuse(why); }
    lopt.colorfile = "run-multi";   // (the coloured run's rules for --model / --filter-multi: the colour file is made here)
    if (!cli.hand_off(mopt.call)) return 1;
    // (--ref-threads is taken and changes nothing, as in the coloured calling run: it writes the `-t 1` text format alone)
    mopt.call.filter_multi = lopt.multi_seen ? &cli.multi : nullptr;
    mopt.call.each_color = lopt.each_color;
    pfh::RunMultiStats st;
    pfh::RunMultiTimes tm;
    string err;
    if (pfh::run_multi_fastq(samples, cli.out, mopt, 0, st, &tm, err)) return cli.failed(err, "ColoredCDBG::read()");
    for (size_t c = 0; c < st.trim.size(); ++c)   // one line per `trim` of the equivalent chain, in the order given
        for (size_t u = 0; u < pfh::trim_unit_count(samples[c].inputs.size(), samples[c].paired); ++u) {
            if (c < st.clip.size() && u < st.clip[c].size()) cerr << pfh::clip_line(st.clip[c][u]) << endl;
            if (c < st.dedup.size() && u < st.dedup[c].size()) cerr << pfh::dedup_line(st.dedup[c][u]) << endl;
            cerr << pfh::trim_unit_line(&st.trim[c][samples[c].paired ? 2 * u : 0], samples[c].paired) << endl;
        }
    cerr << "run-multi: colors " << st.colors << " reads " << st.reads << " bases " << st.bases << " kmers " << st.kmers << " bad " << st.bad << " distinct "
         << st.distinct << " windows_bad " << st.windows_bad << " windows_kept " << st.windows_kept << " distinct_kept " << st.distinct_kept << " unitigs "
         << st.graph.unitigs << " removed " << st.graph.removed << " unitigs_out " << st.graph.unitigs_out << " longest " << st.graph.longest << " kmers_colored "
         << st.kmers_colored << " kmers_unplaced " << st.kmers_unplaced << " runs " << st.runs << " overflow " << st.overflow << " color_bytes " << st.color_bytes << endl;
    for (size_t i = 0; i < st.color.size(); ++i)
        cerr << "run-multi: color " << i << " lower " << st.color[i].lower << " upper " << st.color[i].upper << " distinct " << st.color[i].distinct << " kept "
             << st.color[i].kept << endl;
    if (cli.reads.verbose)
        cerr << "run-multi: count " << tm.count_s << "s db-out " << tm.db_out_s << "s recount " << tm.recount_s << "s union " << tm.union_s << "s graph " << tm.graph_s
             << "s color " << tm.color_s << "s serialise " << tm.serialise_s << "s gfa-out " << tm.gfa_out_s << "s load " << tm.load_s << "s call " << tm.call_s << "s" << endl;
    return 0;
}
