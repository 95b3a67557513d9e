// `ploidyfrost count`, `mask`, `smudge`, `qc` and `trim`: the command lines of the steps in front of the graph
#include <algorithm>
#include <iostream>
#include <string>
#include <vector>

#include "pf_cli.hpp"
#include "pf_cli_subs.hpp"
#include "pf_count_host.hpp"
#include "pf_hetpair_host.hpp"
#include "pf_mask_host.hpp"
#include "pf_qc_host.hpp"
#include "pf_trim_host.hpp"

using namespace std;
using namespace pfcli;

// `count`: step `2.kmc_db` of the reference's workflow (`kmc -ci1 -cs10000 -k25 @FILES kmc_sample tmp`) on the device
int count_main(int argc, char **argv) {
    const Refuse refuse{"count", "Usage:PloidyFrost count -k 25 -ci 1 -cs 10000 [-cx N] [-b] -i reads.fq [-i more.fq ...] -o kmc_database [--hist file] [--chunk-bytes N] [--initial-slots N] [--gz] [--gz-plain] [--fasta] [-v]"};
    CountArgs c;
    ReadsCli reads(ReadsCli::ALL);
    string out;
    vector<string> inputs;
    for (int i = 2; i < argc; ++i) {
        const string a = argv[i];
        string why;
        int taken = c.take(argc, argv, i, why);
        if (!taken) taken = reads.take(argc, argv, i, why);
        if (taken < 0) return refuse(why);
        if (taken) continue;
        if (a != "-i" && a != "-o" && a != "--hist") return refuse("unknown option " + a);
        const char *val = value_of(argc, argv, i, why);
        if (!val) return refuse(why);
        if (a == "-i") inputs.push_back(val);
        else (a == "-o" ? out : c.opt.hist) = val;
    }
    c.opt.gz = reads.gz;
    c.opt.fasta = reads.fasta;
    c.opt.chunk_bytes = reads.chunk_bytes;
    c.opt.initial_slots = reads.initial_slots;
    // refused by name, before anything is read or written
    if (inputs.empty()) return refuse("-i <reads.fq> is missing");
    if (out.empty()) return refuse("-o <KMCDatabase> is missing");
    { const int clause = pfh::count_options_clause(c.opt, true); if (clause) return refuse(pf_count::cut_text(clause)); }
    pf_count_stats st = {};
    pfh::CountTimes tm;
    string err;
    if (pfh::count_fastq(inputs, out, c.opt, 0, st, &tm, err)) return failed(err);
    cerr << "count: reads " << st.reads << " bases " << st.bases << " kmers " << st.kmers << " bad " << st.kmers_bad << " unique " << st.unique << " below "
         << st.below_min << " above " << st.above_max << " written " << st.written << endl;
    if (reads.verbose) cerr << "count: stream " << tm.stream_s << "s finish " << tm.finish_s << "s write " << tm.write_s << "s" << endl;
    return 0;
}

// `mask`: step 2 of the reference's workflow (`kmc_tools filter -hm <db> <reads.fq> -ci<L> <out.fq>`) against the database on the device
// (of the reads options it has -v and a --chunk-bytes of its own wording, so it does not go through ReadsCli)
int mask_main(int argc, char **argv) {
    // (the short form: `--gz-out`, blocked-gzip output, stands in the overall usage)
    const Refuse refuse{"mask", "Usage:PloidyFrost mask -d kmc_database -i reads.fq [-i more.fq ...] -o out.fq (-l L | --auto-cutoffs) [-u U] [--chunk-bytes N] [-v]"};
    string db, out, db_out;
    CountArgs c;   // -k: the inputs are counted instead of a database read
    vector<string> inputs;
    bool l_seen = false, auto_cutoffs = false, verbose = false, gz_out = false;
    long long low = 0, up = 0xFFFFFFFFll, chunk = 0;
    for (int i = 2; i < argc; ++i) {
        const string a = argv[i];
        string why;
        if (const int taken = c.take(argc, argv, i, why)) { if (taken < 0) return refuse(why); continue; }
        if (a == "--auto-cutoffs") { auto_cutoffs = true; continue; }
        if (a == "--gz-out") { gz_out = true; continue; }
        if (a == "--fasta") return refuse("--fasta is not built into mask: the masked output has the input's layout (count, build, build-multi, run and run-multi take FASTA)");
        if (a == "-v") { verbose = true; continue; }
        if (a != "-d" && a != "-i" && a != "-o" && a != "-l" && a != "-u" && a != "--chunk-bytes" && a != "--db-out") return refuse("unknown option " + a);
        const char *val = value_of(argc, argv, i, why);
        if (!val) return refuse(why);
        if (a == "-d") db = val;
        else if (a == "--db-out") db_out = val;
        else if (a == "-i") inputs.push_back(val);
        else if (a == "-o") out = val;
        else if (!ranged(a, val, 0xFFFFFFFFll, a == "-l" ? low : a == "-u" ? up : chunk, why)) return refuse(why);
        else if (a == "-l") l_seen = true;
        else if (a == "--chunk-bytes" && !chunk) return refuse("--chunk-bytes takes a positive number");
    }
    // refused by name, before anything is read or written
    if (!db.empty() && c.k_seen) return refuse("-d does not go with -k (the database is either read, or counted from the inputs)");
    if (!c.k_seen && !c.seen.empty()) return refuse(c.seen + " needs -k (it belongs to the count of the inputs)");
    if (!c.k_seen && !db_out.empty()) return refuse("--db-out needs -k (it belongs to the count of the inputs)");
    if (db.empty() && !c.k_seen) return refuse("-d <KMCDatabase> is missing");
    if (inputs.empty()) return refuse("-i <reads.fq> is missing");
    if (out.empty()) return refuse("-o <out.fq> is missing");
    if (l_seen && auto_cutoffs) return refuse("-l does not go with --auto-cutoffs (the lower threshold is derived: leave it out)");
    if (!l_seen && !auto_cutoffs) return refuse("the lower threshold is missing: -l L, or --auto-cutoffs to derive it from the database");
    if (l_seen && low > up) return refuse("-l " + to_string(low) + " is above -u " + to_string(up) + " (L > U)");
    if (c.k_seen) { const int clause = pfh::count_options_clause(c.opt, !db_out.empty()); if (clause) return refuse(pf_count::cut_text(clause)); }
    pf_mask_stats st = {};
    uint32_t lower = (uint32_t)low;
    pfh::MaskTimes tm;
    string err;
    const int rc = c.k_seen ? pfh::mask_fastq_counted(c.opt, db_out, inputs, out, (uint32_t)low, (uint32_t)up, auto_cutoffs, (uint64_t)chunk, 0, st, lower, &tm, err, gz_out)
                            : pfh::mask_fastq(db, inputs, out, (uint32_t)low, (uint32_t)up, auto_cutoffs, (uint64_t)chunk, 0, st, lower, &tm, err, gz_out);
    if (rc) return failed(err);
    if (auto_cutoffs) cout << lower << endl;   // exactly as `cutoffL -d` prints it
    cerr << "mask: reads " << st.reads << " changed " << st.reads_changed << " bases " << st.bases << " masked " << st.bases_masked << " kmers " << st.kmers
         << " bad " << st.kmers_bad << endl;
    if (verbose)
        cerr << "mask: load " << tm.load_s << "s stream " << tm.stream_s << "s (device " << tm.device_s << "s, read " << tm.read_s << "s, write " << tm.write_s << "s)" << endl;
    return 0;
}

// `smudge`: the Smudgeplot-style check of the ploidy estimate from the k-mer counts on the device (K-HETPAIR, ../pf_hetpair_rule.hpp)
int smudge_main(int argc, char **argv) {
    const Refuse refuse{"smudge", "Usage:PloidyFrost smudge -d kmc_database (-l L -u U | --auto-cutoffs [-q Q]) -o out [-n N] [--pairs FILE] [-v]\n"
                                  "      PloidyFrost smudge -k 25 [-ci 1 -cs 10000 -cx N] -i reads.fq [-i more.fq ...] (-l L -u U | --auto-cutoffs [-q Q]) -o out [-n N] [--pairs FILE]\n"
                                  "                         [--gz | --gz-plain] [--fasta] [--chunk-bytes N] [--initial-slots N] [-v]"};
    string db, out;
    CountArgs c;   // -k: the inputs are counted instead of a database read
    c.opt.ci = 1;  // the workflow's `kmc -ci1 -cs10000`
    c.opt.cs = 10000;
    ReadsCli reads(ReadsCli::GZ | ReadsCli::FASTA);   // (--chunk-bytes and --initial-slots: its own wording, below)
    vector<string> inputs;
    pfh::SmudgeOptions opt;
    bool l_seen = false, u_seen = false, q_seen = false, n_seen = false;
    string reads_option;   // the first option that belongs to the count of the inputs
    long long low = 0, up = 0, n_hap = 0;
    for (int i = 2; i < argc; ++i) {
        const string a = argv[i];
        string why;
        if (const int taken = c.take(argc, argv, i, why)) { if (taken < 0) return refuse(why); continue; }
        if (a == "--auto-cutoffs") { opt.auto_cutoffs = true; continue; }
        if (const int taken = reads.take(argc, argv, i, why)) {
            if (taken < 0) return refuse(why);
            if (reads_option.empty() && a != "-v") reads_option = a;
            continue;
        }
        const bool sizes = a == "--chunk-bytes" || a == "--initial-slots";
        if (!sizes && a != "-d" && a != "-i" && a != "-o" && a != "-l" && a != "-u" && a != "-q" && a != "-n" && a != "--pairs") return refuse("unknown option " + a);
        const char *val = value_of(argc, argv, i, why);
        if (!val) return refuse(why);
        if (a == "-d") db = val;
        else if (a == "-i") { inputs.push_back(val); if (reads_option.empty()) reads_option = a; }
        else if (a == "-o") out = val;
        else if (a == "--pairs") opt.pairs = val;
        else if (a == "-q") {
            try { opt.quantile = stod(val); } catch (const exception &) { return refuse(string("-q takes a quantile below 1, not '") + val + "'"); }
            if (!(opt.quantile > 0) || opt.quantile >= 1) return refuse(string("-q takes a quantile below 1, not '") + val + "'");
            q_seen = true;
        }
        else if (sizes) {
            long long x = 0;
            if (!ranged(a, val, 0x7FFFFFFFFFFFFFFFll, x, why)) return refuse(why);
            if (x < 1) return refuse(a + " takes a positive number");
            (a == "--chunk-bytes" ? c.opt.chunk_bytes : c.opt.initial_slots) = (uint64_t)x;
            if (reads_option.empty()) reads_option = a;
        }
        else if (!ranged(a, val, 0xFFFFFFFFll, a == "-l" ? low : a == "-u" ? up : n_hap, why)) return refuse(why);
        else (a == "-l" ? l_seen : a == "-u" ? u_seen : n_seen) = true;
    }
    c.opt.gz = reads.gz;
    c.opt.fasta = reads.fasta;
    // refused by name, before anything is read or written
    if (!db.empty() && c.k_seen) return refuse("-d does not go with -k (the database is either read, or counted from the inputs)");
    if (db.empty() && !c.k_seen) return refuse("-d <KMCDatabase> or -k <k> with -i <reads.fq> is missing");
    if (!c.k_seen && !c.seen.empty()) return refuse(c.seen + " needs -k (it belongs to the count of the inputs)");
    if (!c.k_seen && !reads_option.empty()) return refuse(reads_option + " needs -k (it belongs to the count of the inputs)");
    if (c.k_seen && inputs.empty()) return refuse("-i <reads.fq> is missing");
    if (out.empty()) return refuse("-o <out> is missing");
    if ((l_seen || u_seen) && opt.auto_cutoffs) return refuse(string(l_seen ? "-l" : "-u") + " does not go with --auto-cutoffs (the bounds are derived: leave it out)");
    if (!opt.auto_cutoffs && !(l_seen && u_seen)) return refuse("the bounds are missing: -l L and -u U, or --auto-cutoffs to derive them from the counts");
    if (q_seen && !opt.auto_cutoffs) return refuse("-q needs --auto-cutoffs (it is the quantile of the derived upper bound)");
    opt.lo = (uint32_t)low;
    opt.hi = (uint32_t)up;
    if (!opt.auto_cutoffs) {
        if (low < 1) return refuse("-l " + to_string(low) + ": " + pf_hetpair::arg_text(pf_hetpair::ARG_LO_ZERO));
        if (low > up) return refuse("-l " + to_string(low) + " is above -u " + to_string(up) + " (L > U)");
        if (up - low + 1 > (long long)pf_hetpair::MAX_W) return refuse("-l " + to_string(low) + " -u " + to_string(up) + ": " + pf_hetpair::arg_text(pf_hetpair::ARG_TOO_WIDE));
    }
    if (n_seen && n_hap < 1) return refuse("-n takes a haploid coverage of at least 1");
    opt.n = (uint64_t)n_hap;
    if (c.k_seen) {
        if (!c.opt.both_strands) return refuse("-b: smudge needs canonical counts");
        const int clause = pfh::count_options_clause(c.opt, false);
        if (clause) return refuse(pf_count::cut_text(clause));
    }
    pfh::SmudgeResult res;
    string err;
    const int rc = c.k_seen ? pfh::smudge_counted(c.opt, inputs, opt, out, 0, res, err) : pfh::smudge_db(db, opt, out, 0, res, err);
    if (rc) return failed(err);
    if (opt.auto_cutoffs) cout << "lower " << res.lo << " upper " << res.hi << endl;
    if (res.clamped) cerr << "smudge: the upper bound was lowered to " << res.hi << " (lower + 4095: the table holds 4096 x 4096 cells)" << endl;
    pf_hetpair::Stats st;
    st.kmers = res.stats.kmers; st.in_range = res.stats.in_range; st.one_partner = res.stats.one_partner; st.many_partners = res.stats.many_partners;
    st.pairs = res.stats.pairs;
    cerr << pf_hetpair::stats_text(st) << endl;
    if (opt.n) cerr << pf_hetpair::proposed_text(res.summary) << endl;
    if (reads.verbose) cerr << "smudge: load " << res.times.load_s << "s pairs " << res.times.pairs_s << "s write " << res.times.write_s << "s" << endl;
    return 0;
}

// `qc`: what FastQC is looked at for before the steps of `trim` are chosen -- quality and base content by cycle, read lengths, the
// quality offset -- from the device, as one tab-separated report (../pf_qc_rule.hpp)
int qc_main(int argc, char **argv) {
    const Refuse refuse{"qc", "Usage:PloidyFrost qc (-i a.fq [-i b.fq ...] | -1 r1.fq [-1 ...] -2 r2.fq [-2 ...]) -o report.tsv [--phred 33|64] [--gz | --gz-plain] [--chunk-bytes N] [-v]"};
    vector<string> inputs, in1, in2;
    string out;
    pfh::QcOptions opt;
    ReadsCli reads(ReadsCli::GZ | ReadsCli::CHUNK);
    PhredCli phred;
    for (int i = 2; i < argc; ++i) {
        const string a = argv[i];
        string why;
        if (a == "--fasta") return refuse("--fasta does not go with qc: FASTA has no qualities to report");
        int taken = reads.take(argc, argv, i, why);
        if (!taken) taken = phred.take(argc, argv, i, why);
        if (taken < 0) return refuse(why);
        if (taken) continue;
        if (a != "-i" && a != "-1" && a != "-2" && a != "-o") return refuse("unknown option " + a);
        const char *val = value_of(argc, argv, i, why);
        if (!val) return refuse(why);
        if (a == "-o") out = val;
        else (a == "-i" ? inputs : a == "-1" ? in1 : in2).push_back(val);
    }
    opt.gz = reads.gz;
    opt.chunk_bytes = reads.chunk_bytes;
    opt.phred = phred.phred;
    // refused by name, before anything is read or written
    if (!inputs.empty() && (!in1.empty() || !in2.empty())) return refuse("-i does not go with -1 / -2 (the inputs are either single-ended or the two sides of pairs)");
    if (inputs.empty() && in1.empty() && in2.empty()) return refuse("-i <reads.fq> is missing (or -1 <r1.fq> -2 <r2.fq>)");
    if (out.empty()) return refuse("-o <report.tsv> is missing");
    pfh::QcReport rep;
    string err;
    if (pfh::qc_fastq(inputs.empty() ? in1 : inputs, in2, out, opt, 0, rep, err)) return failed(err);
    for (const string &l : rep.lines()) cerr << l << endl;
    if (reads.verbose) cerr << "qc: report " << rep.text().size() << " bytes, phred " << rep.phred << " hint " << pf_qc::hint_of(rep.tables.data()) << endl;
    return 0;
}

// `trim`: step 1 of the reference's workflow (`trimmomatic PE -phred33 r1 r2 trim1 u1 trim2 u2 LEADING:10 TRAILING:10 SLIDINGWINDOW:3:20
// MINLEN:50`) on the device; the steps are Trimmomatic's words as positional arguments
int trim_main(int argc, char **argv) {
    const Refuse refuse{"trim", "Usage:PloidyFrost trim -i reads.fq [-i more.fq ...] -o trimmed.fq STEP... [--phred 33|64] [--trimlog file] [--chunk-bytes N] [--gz] [--gz-plain] [--gz-out] [-v]\n"
                                "      PloidyFrost trim -1 r1.fq -2 r2.fq -o1 p1.fq -u1 u1.fq -o2 p2.fq -u2 u2.fq STEP... [the same options]\n"
                                "      STEP: LEADING:t TRAILING:t SLIDINGWINDOW:w:t MINLEN:l\n"
                                "      [--adapters adapters.fa [--adapter-seed 0..8] [--adapter-score 1..1000]]: adapters are clipped first; no STEP is needed beside them\n"
                                "      [--adapter-pairs [--adapter-pair-score 1..1000] [--adapter-pair-min 1..16] [--adapter-keep-both]] with -1 / -2: palindrome mode from the file's Prefix pairs\n"
                                "      [--report report.tsv]: the read quality report of the reads as they come (raw) and as they are written (kept), as `qc` words it"};
    vector<string> inputs, words;
    string out, in_pair[2], out_pair[4];
    pfh::TrimOptions opt;
    ReadsCli reads(ReadsCli::GZ | ReadsCli::CHUNK);
    PhredCli phred;
    ClipCli clip_cli;
    DedupCli dedup_cli;
    const char *pair_opts[6] = {"-1", "-2", "-o1", "-u1", "-o2", "-u2"};
    bool fasta_seen = false;
    // --fasta is refused in front of everything that stands behind it, with --dedup by the pair of options, as run words it
    auto fasta_refusal = [&]() { return refuse(dedup_cli.seen ? "--fasta does not go with --dedup" : "--fasta does not go with trim: FASTA has no qualities to trim"); };
    auto bail = [&](const string &m) { return fasta_seen ? fasta_refusal() : refuse(m); };
    for (int i = 2; i < argc; ++i) {
        const string a = argv[i];
        string why;
        if (a.empty() || a[0] != '-') { words.push_back(a); continue; }
        if (a == "--gz-out") { opt.gz_out = true; continue; }
        if (a == "--fasta") { fasta_seen = true; continue; }   // refused below, worded by what else was given
        int taken = reads.take(argc, argv, i, why);
        if (!taken) taken = clip_cli.take(argc, argv, i, why);
        if (!taken) taken = dedup_cli.take(argc, argv, i, why);
        if (!taken) taken = phred.take(argc, argv, i, why);
        if (taken < 0) return bail(why);
        if (taken) continue;
        const int pair = (int)(std::find_if(pair_opts, pair_opts + 6, [&](const char *o) { return a == o; }) - pair_opts);
        if (pair == 6 && a != "-i" && a != "-o" && a != "--trimlog" && a != "--report") return bail("unknown option " + a);
        const char *val = value_of(argc, argv, i, why);
        if (!val) return bail(why);
        if (a == "-i") inputs.push_back(val);
        else if (a == "-o") out = val;
        else if (a == "--trimlog") opt.trimlog = val;
        else if (a == "--report") { if (!*val) return bail("--report needs a value"); opt.report = val; }
        else (pair < 2 ? in_pair[pair] : out_pair[pair - 2]) = val;
    }
    if (fasta_seen) return fasta_refusal();
    opt.gz = reads.gz;
    opt.chunk_bytes = reads.chunk_bytes;
    opt.phred = phred.phred;
    // refused by name, before anything is read or written
    {
        vector<const char *> w;
        for (const string &x : words) w.push_back(x.c_str());
        vector<pf_trim::Step> steps;
        size_t bad = 0;
        { const string why = clip_cli.finish(opt.clip); if (!why.empty()) return refuse(why); }
        { const string why = dedup_cli.finish(opt.dedup); if (!why.empty()) return refuse(why); }
        const int c = pf_trim::parse_steps(w.data(), w.size(), steps, &bad);
        if (c == pf_trim::REFUSE_NO_STEP && !opt.clip.on() && !opt.dedup.on) return refuse(pf_trim::refusal_text(c));
        if (c && c != pf_trim::REFUSE_NO_STEP) return refuse(words[bad] + ": " + pf_trim::refusal_text(c));
        for (const pf_trim::Step &st : steps) opt.steps.push_back(pf_trim_step{st.kind, st.a, st.b});
    }
    const bool pair_in = !in_pair[0].empty() || !in_pair[1].empty();
    const bool pair_out = !out_pair[0].empty() || !out_pair[1].empty() || !out_pair[2].empty() || !out_pair[3].empty();
    if (!inputs.empty() && pair_in) return refuse("-i does not go with -1 / -2 (the inputs are either single-ended or one pair)");
    if (pair_in && !out.empty()) return refuse("-o does not go with -1 / -2 (a pair is written to -o1 -u1 -o2 -u2)");
    if (opt.clip.on() && opt.clip.pairs && !inputs.empty()) return refuse("--adapter-pairs needs -1 / -2");
    if (!pair_in && pair_out) return refuse(inputs.empty() ? "-1 <r1.fq> and -2 <r2.fq> are missing" : "-o1 -u1 -o2 -u2 do not go with -i (single-ended reads are written to -o)");
    pf_trim_stats st[2] = {};
    pfh::TrimTimes tm;
    pfh::ClipReport clip;
    pfh::QcReport qc;
    pf_dedup_stats dedup = {};
    string err;
    if (pair_in) {
        for (int j = 0; j < 2; ++j)
            if (in_pair[j].empty()) return refuse(string(pair_opts[j]) + " <r" + to_string(j + 1) + ".fq> is missing");
        for (int j = 0; j < 4; ++j)
            if (out_pair[j].empty()) return refuse(string(pair_opts[2 + j]) + " <out.fq> is missing");
        if (pfh::trim_fastq_pair(in_pair[0], in_pair[1], out_pair, opt, 0, st, &tm, err, &clip, &qc, &dedup)) return failed(err);
        if (opt.clip.on()) cerr << pfh::clip_line(clip) << endl;
        if (opt.dedup.on) cerr << pfh::dedup_line(dedup) << endl;
        cerr << "trim: pairs " << st[0].reads << " both " << st[0].both << " forward_only " << st[0].only1 << " reverse_only " << st[0].only2 << " dropped "
             << st[0].neither << " bases " << st[0].bases + st[1].bases << " bases_kept " << st[0].bases_kept + st[1].bases_kept << endl;
    } else {
        if (inputs.empty()) return refuse("-i <reads.fq> is missing (or -1 <r1.fq> -2 <r2.fq> for a pair)");
        if (out.empty()) return refuse("-o <trimmed.fq> is missing");
        if (pfh::trim_fastq(inputs, out, opt, 0, st[0], &tm, err, &clip, &qc, &dedup)) return failed(err);
        if (opt.clip.on()) cerr << pfh::clip_line(clip) << endl;
        if (opt.dedup.on) cerr << pfh::dedup_line(dedup) << endl;
        cerr << "trim: reads " << st[0].reads << " kept " << st[0].kept << " dropped " << st[0].dropped << " bases " << st[0].bases << " bases_kept "
             << st[0].bases_kept << endl;
    }
    for (const string &l : qc.lines()) cerr << l << endl;
    if (reads.verbose) cerr << "trim: stream " << tm.stream_s << "s (device " << tm.device_s << "s, read " << tm.read_s << "s, write " << tm.write_s << "s)" << endl;
    return 0;
}
