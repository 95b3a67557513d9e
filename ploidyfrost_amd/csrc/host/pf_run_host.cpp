#include "pf_run_host.hpp"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <iostream>

#include "pf_cutoffs.hpp"
#include "pf_host_graph.hpp"
#include "../pf_trim_rule.hpp"
#include "pf_host_util.hpp"
#include "pf_trim_host.hpp"

namespace pfh {

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

CountOptions count_options_of(const RunOptions &opt) {
    CountOptions c;
    c.k = opt.k;
    c.ci = opt.ci;
    c.cx = opt.cx;
    c.cs = opt.cs;
    c.both_strands = true;
    c.chunk_bytes = opt.chunk_bytes;
    c.initial_slots = opt.initial_slots;
    return c;
}

}  // namespace

// ---- the calling run behind a loaded CDBG ----
int call_configure(CDBG &g, const CallSetup &s) {
    g.set_threads((unsigned)s.threads);
    g.set_overlap_output(true);
    if (s.ref_threads > 1 && g.set_reference_threads(s.ref_threads)) return 1;
    if (getenv("PF_BFS_HUGE_ON_DEVICE")) g.set_third_tier_on_host(false);   // experiments: giant traversals on one wavefront each
    return 0;
}

int call_run(CDBG &g, const CallSetup &s, const std::function<void(const char *)> &mark) {
    auto done = [&](const char *what) { if (mark) mark(what); };
    if (s.model.on && g.set_model(s.model)) return 1;
    if (s.filter && g.set_filter(s.filter)) return 1;
    if (s.density_points && g.set_density(s.density_points, s.density_adjust)) return 1;
    if (g.setUnitigId(s.outprefix, "", s.threads)) return 1;
    if (s.info && g.printInfo(s.verbose, s.outprefix)) return 1;
    done("setUnitigId");
    if (g.findSuperBubble_multithread_ptr(s.outprefix, s.threads)) return 1;
    done("findSuperBubble");
    std::cout << "CDBG:: Minimum Coverage:" << s.lower << std::endl;
    std::cout << "CDBG:: Maximum Coverage:" << s.upper << std::endl;
    if (g.ploidyEstimation_multithread_ptr(s.outprefix, s.lower, s.upper, s.threads)) return 1;
    done("PloidyEstimation");
    if (s.model.on) std::cout << g.model_last_line() << std::endl;
    if (s.verbose) {
        const PhaseTimes &t = g.times();
        printf("[device] candidates %llu (big tier %llu)  bfs %.3fs replay %.3fs | cov %.3fs tasks %.3fs (%llu) align %.3fs (%llu jobs) "
               "sites %.3fs (%llu strings) format %.3fs write %.3fs\n",
               (unsigned long long)t.candidates, (unsigned long long)t.bfs_deferred, t.bfs_device_s, t.replay_s, t.cov_device_s,
               t.tasks_s, (unsigned long long)t.tasks, t.align_s, (unsigned long long)t.align_jobs, t.sites_s,
               (unsigned long long)t.site_strings, t.format_s, t.write_s);
        printf("[bfs]    traversals > 4096 unitigs: %llu (sum of seen %llu, largest %llu); committed by the replay: %llu (largest %llu)\n",
               (unsigned long long)t.bfs_large, (unsigned long long)t.bfs_large_seen, (unsigned long long)t.bfs_max_seen,
               (unsigned long long)t.bfs_large_used, (unsigned long long)t.bfs_large_used_max);
        printf("[host]   scan %.3fs | align: build %.3fs device-call %.3fs post %.3fs choose %.3fs\n", t.scan_s, t.align_build_s,
               t.align_device_s, t.align_post_s, t.align_choose_s);
    }
    return 0;
}

// ---- the coloured calling run behind a loaded CCDBG ----
int colored_call_run(CCDBG &g, ColoredCallSetup &s, std::string &err) {
    using std::cerr;
    using std::cout;
    using std::endl;
    if (s.color_rows) {   // one (lower, upper) per colour from its own database, as -h derives them from one file per colour (src/Main.cpp:359-396)
        for (size_t c = 0; c < s.color_rows->size() && c < s.cutoffs.size(); c++) {
            int lo = 0, hi = 0;
            if (cutoffs_from_rows((*s.color_rows)[c], s.quantile, lo, hi)) { err = "Error: Histogram File is badly Formatted."; return 1; }
            s.cutoffs[c] = {std::max(10, lo), hi};
            if (s.cutoffs[c].first > s.cutoffs[c].second) { err = "Error: lower cutoff need be smaller than upper cutoff "; return 1; }
        }
    }
    auto bad = [&]() { err = g.error(); return 1; };
    g.set_threads((unsigned)s.threads);
    g.set_overlap_output(true);
    if (s.model.on && g.set_model(s.model)) return bad();
    if (s.filter_multi && g.set_filter_multi(s.filter_multi, s.each_color)) return bad();
    if (s.density_points && g.set_density(s.density_points, s.density_adjust)) return bad();
    if (g.setUnitigId(s.outprefix, s.graphfile, s.threads)) return bad();
    if (s.info && g.printInfo(s.verbose, s.outprefix)) return bad();
    if (g.findSuperBubble_multithread_ptr(s.outprefix, s.threads)) return bad();
    for (size_t i = 0; i < s.cutoffs.size(); i++) {
        cout << "CCDBG:: Database " << i << " Minimum Coverage:" << s.cutoffs[i].first << endl;
        cout << "CCDBG:: Maximum Coverage:" << s.cutoffs[i].second << endl;
    }
    if (g.ploidyEstimation_multithread_ptr(s.outprefix, s.cutoffs, s.threads)) return bad();
    if (s.model.on && s.each_color) {
        for (int c : g.model_colors_without_rows()) cerr << "color " << c << ": no row kept, no estimate" << endl;
        for (int c : g.model_colors_without_values()) cerr << "color " << c << ": the rows kept hold no value for the model, no estimate" << endl;
        for (const CDBG::ColorFit &cf : g.model_color_fits()) cout << "color " << cf.color << ": estimated ploidy level is : " << cf.ploidy << endl;
        for (int c : g.model_colors_without_density()) cerr << "color " << c << ": need at least 2 data points, no density" << endl;
    } else if (s.model.on) cout << g.model_last_line() << endl;
    if (s.verbose) {
        const PhaseTimes &t = g.times();
        printf("[device] candidates %llu  bfs %.3fs replay %.3fs | cov %.3fs tasks %.3fs (%llu) align %.3fs (%llu jobs) "
               "sites %.3fs (%llu strings) format %.3fs write %.3fs\n",
               (unsigned long long)t.candidates, t.bfs_device_s, t.replay_s, t.cov_device_s, t.tasks_s, (unsigned long long)t.tasks,
               t.align_s, (unsigned long long)t.align_jobs, t.sites_s, (unsigned long long)t.site_strings, t.format_s, t.write_s);
    }
    return 0;
}

// ---- trimmed inputs ----
std::string trim_inputs_refusal(const std::vector<std::string> &inputs, bool paired, const TrimInputs &trim) {
    if (paired && !trim.on()) return "the files of a pair are trimmed together: -1 / -2 need a step (two files without trimming go with -i)";
    if (!trim.on()) return "";
    if (trim.clip.on() && trim.clip.pairs && !paired) return "--adapter-pairs needs -1 / -2";
    {
        TrimOptions o;
        o.steps = trim.steps;
        o.phred = trim.phred;
        o.clip = trim.clip;
        o.dedup = trim.dedup;
        std::string e;
        if (trim_options_clause(o, e)) return e.substr(6);   // (worded "trim: ...": the caller puts its own name in front)
    }
    if (paired && inputs.size() % 2) return inputs.back() + ": the first file of a pair without its second (-1 <r1.fq> -2 <r2.fq>)";
    for (size_t i = 0; i < inputs.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if (same_file(inputs[i], inputs[j]))
                return inputs[i] + (inputs[i] == inputs[j] ? " is given twice" : " and " + inputs[j] + " are one file") + ": every read is counted once";
    return "";
}

std::string trim_unit_line(const pf_trim_stats *st, bool paired) {
    auto n = [](uint64_t v) { return std::to_string(v); };
    if (paired)
        return "trim: pairs " + n(st[0].reads) + " both " + n(st[0].both) + " forward_only " + n(st[0].only1) + " reverse_only " + n(st[0].only2) + " dropped " +
               n(st[0].neither) + " bases " + n(st[0].bases + st[1].bases) + " bases_kept " + n(st[0].bases_kept + st[1].bases_kept);
    return "trim: reads " + n(st[0].reads) + " kept " + n(st[0].kept) + " dropped " + n(st[0].dropped) + " bases " + n(st[0].bases) + " bases_kept " +
           n(st[0].bases_kept);
}

namespace {
void add_masked_stats(pf_maskcount_stats &a, const pf_maskcount_stats &b) {
    a.reads += b.reads; a.bases += b.bases; a.kmers += b.kmers; a.kmers_invalid += b.kmers_invalid; a.kmers_bad += b.kmers_bad; a.kmers_kept += b.kmers_kept;
}
}  // namespace

int stream_trimmed(pf_ctx *ctx, const char *who, const std::vector<ReadsInput> &inputs, bool paired, const TrimInputs &trim, uint64_t chunk_bytes,
                   bool masked, uint32_t low, uint32_t up, pf_trim_stats *unit_stats, pf_maskcount_stats *masked_stats, std::string &err,
                   ClipCounts *unit_clip, pf_dedup_stats *unit_dedup) {
    const pf_trim_plan plan = {trim.steps.data(), (uint32_t)trim.steps.size(), trim.phred};
    // what the clip has counted since the last unit ended, into unit u
    ClipCounts clip_seen;
    auto clip_unit = [&](size_t u, bool store) {
        if (!unit_clip) return 0;
        ClipCounts now;
        if (clip_counts(ctx, trim.clip.pairs, now) != PF_OK) { err = std::string(who) + ": " + pf_last_error(ctx); return 1; }
        if (store) unit_clip[u] = clip_counts_since(now, clip_seen);
        clip_seen = now;
        return 0;
    };
    if (clip_unit(0, false)) return 1;
    // --dedup: one table per unit, as one `trim --dedup` command of the equivalent chain has
    auto dedup_begin = [&]() {
        if (dedup_open(ctx, trim.dedup) == PF_OK) return 0;
        err = std::string(who) + ": " + pf_last_error(ctx);
        return 1;
    };
    auto dedup_end = [&](size_t u) {
        if (dedup_close(ctx, trim.dedup, unit_dedup ? &unit_dedup[u] : nullptr) == PF_OK) return 0;
        err = std::string(who) + ": " + pf_last_error(ctx);
        return 1;
    };
    if (!paired) {
        if (dedup_begin()) return 1;
        StreamTimes stm;
        const int rc0 = stream_fastq(ctx, who, inputs, chunk_bytes, -1, "",
                            [&](const Chunk &c, Taken &t) {
                                pf_trim_stats ts = {};
                                pf_count_stats cs = {};
                                pf_maskcount_stats ms = {};
                                const int rc = masked ? pf_maskcount_fastq_trimmed(ctx, c.text, c.n, c.final ? 1 : 0, &plan, low, up, &t.used, &ts, &ms, &t.bad)
                                                      : pf_count_fastq_trimmed(ctx, c.text, c.n, c.final ? 1 : 0, &plan, &t.used, &ts, &cs, &t.bad);
                                if (rc != PF_OK) return rc;
                                t.reads = ts.reads;   // the records taken, kept or not: the next chunk's records are numbered behind them
                                if (unit_stats) add_trim_stats(unit_stats[0], ts);
                                if (masked_stats) add_masked_stats(*masked_stats, ms);
                                return (int)PF_OK;
                            },
                            stm, err);
        if (rc0) { if (trim.dedup.on) (void)pf_dedup_end(ctx); return rc0; }
        return dedup_end(0) ? 1 : clip_unit(0, true);
    }
    for (size_t u = 0; u + 1 < inputs.size(); u += 2) {
        if (dedup_begin()) return 1;
        PairStreamTimes ptm;
        if (stream_fastq_pair(ctx, who, inputs[u], inputs[u + 1], chunk_bytes,
                              [&](const PairChunk &c, PairTaken &t) {
                                  pf_trim_stats ts[2] = {};
                                  pf_count_stats cs = {};
                                  pf_maskcount_stats ms = {};
                                  const int rc = masked ? pf_maskcount_fastq_pair_trimmed(ctx, c.text[0], c.n[0], c.text[1], c.n[1], c.final ? 1 : 0, &plan, low, up,
                                                                                          t.used, ts, &ms, &t.bad)
                                                        : pf_count_fastq_pair_trimmed(ctx, c.text[0], c.n[0], c.text[1], c.n[1], c.final ? 1 : 0, &plan, t.used, ts, &cs,
                                                                                      &t.bad);
                                  if (rc != PF_OK) return rc;
                                  t.reads = ts[0].reads;
                                  if (unit_stats) { add_trim_stats(unit_stats[u], ts[0]); add_trim_stats(unit_stats[u + 1], ts[1]); }
                                  if (masked_stats) add_masked_stats(*masked_stats, ms);
                                  return (int)PF_OK;
                              },
                              ptm, err)) {
            if (trim.dedup.on) (void)pf_dedup_end(ctx);
            return 1;
        }
        if (dedup_end(u / 2) || clip_unit(u / 2, true)) return 1;
    }
    return 0;
}

// ---- run ----
std::string run_options_refusal(const RunOptions &opt) {
    if (opt.fasta && !opt.report.empty()) return "--fasta does not go with --report (FASTA has no qualities to report)";
    if (!opt.report.empty() && !opt.trim.on()) return "--report needs a step or --adapters in run: ploidyfrost qc reports on files as they are";
    if (!opt.smudge && opt.smudge_n_seen) return "--smudge-n needs --smudge (it is the haploid coverage of the k-mer pair report)";
    if (!opt.smudge && !opt.smudge_pairs.empty()) return "--smudge-pairs needs --smudge (it is the pairs file of the k-mer pair report)";
    if (opt.smudge && opt.smudge_n_seen && opt.smudge_n < 1) return "--smudge-n takes a haploid coverage of at least 1";
    if (opt.fasta && opt.trim.dedup.on) return "--fasta does not go with --dedup";
    if (opt.fasta && opt.trim.clip.on()) return "--fasta does not go with --adapters (FASTA has no qualities to score an adapter by)";
    if (opt.fasta && (opt.trim.on() || opt.paired)) return "--fasta does not go with trim steps or -1 / -2 (FASTA has no qualities to trim)";
    { const int c = count_options_clause(count_options_of(opt), true); if (c) return pf_count::cut_text(c); }
    BuildOptions b;
    b.k = opt.k;
    b.g = opt.g;
    return build_options_refusal(b);
}

int run_fastq(const std::vector<std::string> &inputs, const std::string &out_prefix, const RunOptions &opt, int device, RunStats &stats, RunTimes *times,
              std::string &err) {
    stats = RunStats{};
    RunTimes tm;
    // ---- refusals that need no device ----
    if (inputs.empty()) { err = "run: no input"; return 1; }
    if (out_prefix.empty()) { err = "run: no output prefix"; return 1; }
    { const std::string why = run_options_refusal(opt); if (!why.empty()) { err = "run: " + why; return 1; } }
    { const std::string why = trim_inputs_refusal(inputs, opt.paired, opt.trim); if (!why.empty()) { err = "run: " + why; return 1; } }
    const bool trimming = opt.trim.on();
    if (trimming) stats.trim.assign(opt.paired ? inputs.size() : 1, pf_trim_stats{});
    const CountOptions copt = count_options_of(opt);
    const std::string tail = ".tmp." + std::to_string((long)getpid());
    const std::string gfa_path = opt.gfa_out.empty() ? "" : opt.gfa_out + ".gfa", gfa_tmp = gfa_path + tail;
    std::vector<std::string> outputs;
    if (!opt.db_out.empty()) { outputs.push_back(opt.db_out + ".kmc_pre"); outputs.push_back(opt.db_out + ".kmc_suf"); }
    if (!gfa_path.empty()) outputs.push_back(gfa_path);
    const std::string report_tmp = opt.report + tail;
    if (!opt.report.empty()) {
        for (const std::string &o : outputs)
            if (same_file(o, opt.report)) { err = "run: two outputs have the same path (" + opt.report + ")"; return 1; }
        outputs.push_back(opt.report);
    }
    // --smudge: the report goes beside the calling run's files, the pairs file where it is asked for
    const std::string smudge_path = opt.smudge ? "PloidyFrost_output/" + smudge_report_path(out_prefix) : "", smudge_tmp = smudge_path + tail;
    const std::string pairs_tmp = opt.smudge_pairs + tail;
    if (opt.smudge) {
        for (const std::string &p : {smudge_path, opt.smudge_pairs}) {
            if (p.empty()) continue;
            for (const std::string &o : outputs)
                if (o == p || same_file(o, p)) { err = "run: two outputs have the same path (" + p + ")"; return 1; }
            outputs.push_back(p);
        }
    }
    std::string smudge_text;
    std::vector<ReadsInput> reads;   // what each input is: decided here, once, for both passes
    if (fastq_preflight("run", "read", inputs, outputs, ReadsOptions{opt.gz, opt.fasta}, reads, err)) return 1;
    pf_clip::Adapters adapters;   // --adapters: read and refused here, before a device context exists
    if (opt.trim.clip.on() && clip_load(opt.trim.clip, adapters, err)) { err = "run: " + err; return 1; }

    pf_ctx *ctx = nullptr;
    if (pf_create(device, &ctx) != PF_OK) {
        err = std::string("run: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); reads are counted and called on the GPU only";
        return 1;
    }
    // (the context goes to the loader of the calling run in the end: destroyed here only on the way out before that)
    CtxGuard ctx_guard{ctx};
    bool db_written = false, gfa_tmp_written = false, report_tmp_written = false, pairs_tmp_written = false, smudge_tmp_written = false;
    auto fail = [&](const std::string &m) {   // nothing is left under any output name after a refusal
        err = m;
        if (db_written) { unlink((opt.db_out + ".kmc_pre").c_str()); unlink((opt.db_out + ".kmc_suf").c_str()); }
        if (gfa_tmp_written) unlink(gfa_tmp.c_str());
        if (report_tmp_written) unlink(report_tmp.c_str());
        if (pairs_tmp_written) unlink(pairs_tmp.c_str());
        if (smudge_tmp_written) unlink(smudge_tmp.c_str());
        return 1;
    };
    auto dev_fail = [&]() { return fail(std::string("run: ") + pf_last_error(ctx)); };
    std::vector<ClipCounts> unit_clip;
    if (opt.trim.clip.on()) {   // the clip stays open over both passes; the first one is reported
        if (clip_open(ctx, adapters, opt.trim.clip) != PF_OK) return dev_fail();
        unit_clip.assign(trim_unit_count(inputs.size(), opt.paired), ClipCounts{});
    }
    if (!opt.report.empty() && qc_open(ctx, opt.trim.phred, "run", err)) return 1;   // open over the first pass alone
    if (opt.trim.dedup.on) stats.dedup.assign(trim_unit_count(inputs.size(), opt.paired), pf_dedup_stats{});   // (both passes decide alike; the first is reported)

    // ---- count: every k-mer of the reads, both strands, the user's cut-offs ----
    std::vector<uint64_t> rows;
    int lo = 0, hi = 0;   // L, U
    {
        Counted db;
        CountTimes ctm;
        if (trimming ? count_stream_with(ctx, "run", copt, [&](std::string &e) {
                           return stream_trimmed(ctx, "run", reads, opt.paired, opt.trim, opt.chunk_bytes, false, 0, 0, stats.trim.data(), nullptr, e,
                                                 unit_clip.empty() ? nullptr : unit_clip.data(), stats.dedup.empty() ? nullptr : stats.dedup.data());
                       }, db, stats.counted, ctm, err)
                     : count_stream(ctx, "run", reads, copt, db, stats.counted, ctm, err))
            return 1;
        if (!opt.report.empty()) {   // closed before the second pass streams the same records again
            if (qc_close(ctx, opt.trim.phred, opt.trim.clip.on(), "run", stats.qc, err)) return fail(err);
            const std::string text = stats.qc.text();
            const int fd = open(report_tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            if (fd < 0) return fail("run: cannot write " + report_tmp + " (" + strerror(errno) + ")");
            report_tmp_written = true;
            if (!write_all(fd, text.data(), text.size())) { const int e = errno; close(fd); return fail("run: writing " + report_tmp + " (" + strerror(e) + ")"); }
            if (close(fd) != 0) return fail("run: closing " + report_tmp + " (" + strerror(errno) + ")");
        }
        struct Free { pf_ctx *c; Counted &d; ~Free() { pf_device_free(c, d.kmers); pf_device_free(c, d.counts); } } free_db{ctx, db};
        tm.count_s = ctm.stream_s;
        tm.finish_s = ctm.finish_s;
        // ---- cut-offs and the table: the histogram rows of the finished counters, then the counters into the table ----
        const auto t_table = clk::now();
        if (counted_rows(ctx, db, copt, rows) != PF_OK) return fail(std::string("run: histogram of the counters: ") + pf_last_error(ctx));
        if (cutoffs_from_rows(rows, opt.quantile, lo, hi)) return fail("Error: Histogram File is badly Formatted.");
        lo = std::max(10, lo);   // (what the calling run refuses about the pair it refuses below, where the chain's last command does)
        stats.lower = (uint32_t)lo;
        stats.upper = (uint32_t)std::max(hi, 0);
        if (stats.lower > opt.mask_up)
            return fail("run: the derived lower threshold " + std::to_string(stats.lower) + " is above the upper threshold " + std::to_string(opt.mask_up));
        printf("%u\n", stats.lower);   // exactly as `mask --auto-cutoffs` prints it
        fflush(stdout);
        if (pf_upload_counts(ctx, db.kmers, db.counts, db.n, opt.k, opt.ci, opt.cx, 1) != PF_OK)
            return fail(std::string("run: count table of the inputs: ") + pf_last_error(ctx));
        tm.table_s = since(t_table);
        if (opt.smudge) {   // arrays and table are both alive here: the cross-check costs no pass over the reads
            const auto t_smudge = clk::now();
            const uint32_t s_lo = stats.lower, s_hi = (uint32_t)std::min<uint64_t>(stats.upper, (uint64_t)s_lo + pf_hetpair::MAX_W - 1);
            if (s_lo > stats.upper) return fail("run: --smudge: the lower threshold " + std::to_string(s_lo) + " is above the upper threshold " + std::to_string(stats.upper));
            if (s_hi != stats.upper)
                fprintf(stderr, "run: smudge: the upper bound was lowered from %u to %u (lower + 4095: the table holds 4096 x 4096 cells)\n", stats.upper, s_hi);
            int pairs_fd = -1;
            if (!opt.smudge_pairs.empty()) {
                pairs_fd = open(pairs_tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
                if (pairs_fd < 0) return fail("run: cannot write " + pairs_tmp + " (" + strerror(errno) + ")");
                pairs_tmp_written = true;
            }
            std::string e;
            const int rc = smudge_resident(ctx, "run", db.kmers, db.counts, db.n, opt.k, s_lo, s_hi, opt.smudge_n, pairs_fd, pairs_tmp, stats.smudge, smudge_text, e);
            if (pairs_fd >= 0 && close(pairs_fd) != 0 && !rc) return fail("run: closing " + pairs_tmp + " (" + strerror(errno) + ")");
            if (rc) return fail(e);
            stats.smudge.clamped = s_hi != stats.upper;
            tm.smudge_s = since(t_smudge);
        }
        if (!opt.db_out.empty()) {
            const auto t_db = clk::now();
            if (write_counted(ctx, "run", opt.db_out, db, copt, err)) return fail(err);
            db_written = true;
            tm.db_out_s = since(t_db);
        }
    }   // (the first count's arrays are freed here: the table holds what the rest of the run asks for)

    // ---- recount: the k-mers of the masked reads, without the masked reads ----
    Counted kept;
    struct FreeKept { pf_ctx *&c; Counted &d; ~FreeKept() { if (c) { pf_device_free(c, d.kmers); pf_device_free(c, d.counts); } } } free_kept{ctx_guard.c, kept};
    {
        const auto t_stream = clk::now();
        if (pf_count_begin(ctx, opt.k, 1, opt.initial_slots) != PF_OK) return dev_fail();
        StreamTimes stm;
        if (trimming ? stream_trimmed(ctx, "run", reads, opt.paired, opt.trim, opt.chunk_bytes, true, stats.lower, opt.mask_up, nullptr, &stats.masked, err)
                     : stream_fastq(ctx, "run", reads, opt.chunk_bytes, -1, "",
                         [&](const Chunk &c, Taken &t) {
                             pf_maskcount_stats st = {};
                             const int rc = c.fasta ? pf_maskcount_fasta(ctx, c.text, c.n, c.final ? 1 : 0, stats.lower, opt.mask_up, &t.used, &st, &t.bad)
                                                    : pf_maskcount_fastq(ctx, c.text, c.n, c.final ? 1 : 0, stats.lower, opt.mask_up, &t.used, &st, &t.bad);
                             if (rc != PF_OK) return rc;
                             t.reads = st.reads;
                             add_masked_stats(stats.masked, st);
                             return (int)PF_OK;
                         },
                         stm, err)) {
            pf_count_abort(ctx);
            return fail(err);
        }
        tm.recount_s = since(t_stream);
        const auto t_finish = clk::now();
        pf_count_stats st2 = {};
        if (pf_count_finish(ctx, 1, pf_count::COUNTER_MAX, pf_count::COUNTER_MAX, &kept.kmers, &kept.counts, &kept.n, &st2) != PF_OK) {
            const int rc = dev_fail();
            pf_count_abort(ctx);
            return rc;
        }
        tm.refinish_s = since(t_finish);
        pf_device_free(ctx, kept.counts);   // the graph asks for the k-mers alone
        kept.counts = nullptr;
        stats.distinct_kept = kept.n;
    }
    if (opt.trim.clip.on()) {
        for (const ClipCounts &u : unit_clip) stats.clip.push_back(clip_report_of(adapters, opt.trim.clip, u));
        if (pf_clip_end(ctx) != PF_OK) return dev_fail();
    }
    if (kept.n >= pf_unitig::MAX_KMERS) return fail(std::string("run: ") + pf_unitig::TOO_MANY_TEXT + " (" + std::to_string(kept.n) + ")");

    // ---- graph ----
    const auto t_graph = clk::now();
    const uint32_t g = opt.g == BuildOptions::G_DEFAULT ? PF_UNITIG_G_DEFAULT : (uint32_t)opt.g;
    if (pf_unitig_build(ctx, kept.kmers, kept.n, opt.k, g, opt.clip_tips ? 1 : 0, opt.del_isolated ? 1 : 0, &stats.graph) != PF_OK) return dev_fail();
    pf_device_free(ctx, kept.kmers);   // the second count's arrays are dead: the text is the graph
    kept.kmers = nullptr;
    tm.graph_s = since(t_graph);

    // ---- hand-off: the text stays where it is; the host gets its one copy (the size of the graph, not of the reads) ----
    const auto t_load = clk::now();
    const char *dev_text = nullptr;
    uint64_t n_text = 0;
    if (pf_unitig_text(ctx, &dev_text, &n_text) != PF_OK) return dev_fail();
    std::vector<char> host_text((size_t)n_text);
    if (pf_unitig_fetch(ctx, 0, n_text, host_text.data()) != PF_OK) return dev_fail();
    if (!gfa_path.empty()) {
        const auto t_gfa = clk::now();
        const int fd = open(gfa_tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) return fail("run: cannot write " + gfa_tmp + " (" + strerror(errno) + ")");
        gfa_tmp_written = true;
        if (!write_all(fd, host_text.data(), n_text)) { const int e = errno; close(fd); return fail("run: writing " + gfa_tmp + " (" + strerror(e) + ")"); }
        if (close(fd) != 0) return fail("run: closing " + gfa_tmp + " (" + strerror(errno) + ")");
        tm.gfa_out_s = since(t_gfa);
    }
    UnitigSet graph;
    {
        std::string e;
        if (!graph.open_gfa_memory(host_text.data(), n_text, dev_text, e)) return fail("CompactedDBG::read(): Graph could not be loaded! Exit. (" + e + ")");
    }
    graph.parse_on_device(ctx);   // a refusal is reported by the constructor
    CountsLoader counts;
    counts.adopt(ctx, (int)opt.k, true, rows, opt.ci);
    ctx_guard.c = nullptr;   // the loader's from here, then the CDBG's
    double match = opt.match, mismatch = opt.mismatch, gap = opt.gap;
    const size_t complex_size = opt.complex_size;
    CDBG cdbg(graph, complex_size, match, mismatch, gap, "", device, false, &counts);
    if (!cdbg.good()) return fail(cdbg.error());
    // as --auto-cutoffs checks the pair once graph and table are loaded
    if (lo < 0 || hi < 0) return fail("Error: Filter coverage need a positive number.");
    if (lo > hi) return fail("Error: lower cutoff need be smaller than upper cutoff ");
    tm.load_s = since(t_load) - tm.gfa_out_s;

    // ---- calling: the single-sample path as the command line sets it up ----
    const auto t_call = clk::now();
    CallSetup call = opt.call;
    call.outprefix = out_prefix;
    call.lower = (int)stats.lower;
    call.upper = (int)stats.upper;
    if (call_configure(cdbg, call) || call_run(cdbg, call)) return fail(cdbg.error());
    stats.model_last_line = cdbg.model_last_line();
    tm.call_s = since(t_call);
    if (!gfa_path.empty() && rename(gfa_tmp.c_str(), gfa_path.c_str()) != 0)
        return fail("run: renaming " + gfa_tmp + " to " + gfa_path + " (" + strerror(errno) + ")");
    if (!opt.report.empty() && rename(report_tmp.c_str(), opt.report.c_str()) != 0)
        return fail("run: renaming " + report_tmp + " to " + opt.report + " (" + strerror(errno) + ")");
    if (opt.smudge) {   // the directory is the calling run's: it exists by now
        const int fd = open(smudge_tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) return fail("run: cannot write " + smudge_tmp + " (" + strerror(errno) + ")");
        smudge_tmp_written = true;
        if (!write_all(fd, smudge_text.data(), smudge_text.size())) { const int e = errno; close(fd); return fail("run: writing " + smudge_tmp + " (" + strerror(e) + ")"); }
        if (close(fd) != 0) return fail("run: closing " + smudge_tmp + " (" + strerror(errno) + ")");
        if (rename(smudge_tmp.c_str(), smudge_path.c_str()) != 0) return fail("run: renaming " + smudge_tmp + " to " + smudge_path + " (" + strerror(errno) + ")");
        if (!opt.smudge_pairs.empty() && rename(pairs_tmp.c_str(), opt.smudge_pairs.c_str()) != 0)
            return fail("run: renaming " + pairs_tmp + " to " + opt.smudge_pairs + " (" + strerror(errno) + ")");
    }
    fflush(stdout);
    if (times) *times = tm;
    return 0;
}

}  // namespace pfh
