#include "pf_runmulti_host.hpp"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <iostream>

#include "../pf_runmulti_rule.hpp"
#include "pf_bfg_write.hpp"
#include "pf_cutoffs.hpp"
#include "pf_host_graph.hpp"
#include "pf_host_util.hpp"

namespace pfh {

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

bool write_file(const std::string &path, const void *p, uint64_t n, std::string &why) {
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) { why = "cannot write " + path + " (" + strerror(errno) + ")"; return false; }
    const char *c = static_cast<const char *>(p);
    for (uint64_t done = 0; done < n;) {
        const ssize_t put = write(fd, c + done, (size_t)(n - done));
        if (put < 0 && errno == EINTR) continue;
        if (put < 0) { why = "writing " + path + " (" + strerror(errno) + ")"; close(fd); return false; }
        done += (uint64_t)put;
    }
    if (close(fd) != 0) { why = "closing " + path + " (" + strerror(errno) + ")"; return false; }
    return true;
}

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

// device arrays that die with the scope unless the context has been handed on (ctx = nullptr: its new owner frees them by hand or
// with the context)
struct DeviceArrays {
    pf_ctx *&ctx;
    std::vector<void *> p;
    explicit DeviceArrays(pf_ctx *&c) : ctx(c) {}
    void drop(void *q, pf_ctx *with) {
        if (!q) return;
        pf_device_free(with, q);
        for (void *&x : p) if (x == q) x = nullptr;
    }
    ~DeviceArrays() { if (ctx) for (void *x : p) pf_device_free(ctx, x); }
};

}  // namespace

std::string run_multi_samples_refusal(const std::vector<MultiSample> &samples) {
    if (samples.empty()) return "no sample (--sample NAME -i reads.fq ...)";
    if (samples.size() > pf_runmulti::MAX_SETS) return std::string(pf_runmulti::TOO_MANY_SAMPLES_TEXT) + ": " + std::to_string(samples.size());
    for (size_t c = 0; c < samples.size(); ++c) {
        if (samples[c].name.empty()) return "sample " + std::to_string(c) + " has no name";
        if (samples[c].name.find('\n') != std::string::npos) return "sample " + std::to_string(c) + ": a name holds no line break";
        if (samples[c].inputs.empty()) return "sample " + samples[c].name + " has no input (-i reads.fq behind --sample " + samples[c].name + ")";
        for (size_t d = 0; d < c; ++d)
            if (samples[d].name == samples[c].name) return "sample " + samples[c].name + " is given twice: a colour is a sample";
    }
    for (size_t c = 0; c < samples.size(); ++c)
        for (size_t d = 0; d < c; ++d)
            for (const std::string &a : samples[c].inputs)
                for (const std::string &b : samples[d].inputs)
                    if (a == b) return a + ": the same file is given in two samples (" + samples[d].name + " and " + samples[c].name + ")";
    return "";
}

int run_multi_fastq(const std::vector<MultiSample> &samples, const std::string &out_prefix, const RunMultiOptions &mopt, int device, RunMultiStats &stats,
                    RunMultiTimes *times, std::string &err) {
    stats = RunMultiStats{};
    RunMultiTimes tm;
    const RunOptions &opt = mopt.run;
    const uint32_t n_seeds = mopt.n_seeds ? mopt.n_seeds : pf_color::DEFAULT_SEEDS;
    // ---- refusals that need no device ----
    { const std::string why = run_multi_samples_refusal(samples); if (!why.empty()) { err = "run-multi: " + why; return 1; } }
    if (out_prefix.empty()) { err = "run-multi: no output prefix"; return 1; }
    { const std::string why = run_options_refusal(opt); if (!why.empty()) { err = "run-multi: " + why; return 1; } }
    if (!pf_color::seeds_ok(n_seeds)) { err = "run-multi: " + pf_color::seeds_text(); return 1; }
    const bool trimming = opt.trim.on();
    for (const MultiSample &s : samples) {   // (the steps and the offset are global: they are refused with the first sample)
        const std::string why = trim_inputs_refusal(s.inputs, s.paired, opt.trim);
        if (!why.empty()) { err = "run-multi: sample " + s.name + ": " + why; return 1; }
    }
    const uint32_t C = (uint32_t)samples.size();
    const CountOptions copt = count_options_of(opt);
    const std::string tail = ".tmp." + std::to_string((long)getpid());
    const std::string gfa_path = opt.gfa_out.empty() ? "" : opt.gfa_out + ".gfa", col_path = opt.gfa_out.empty() ? "" : opt.gfa_out + ".bfg_colors";
    const std::string gfa_tmp = gfa_path + tail, col_tmp = col_path + tail;
    std::vector<std::string> outputs, all_inputs, names;
    for (uint32_t c = 0; c < C; ++c) {
        names.push_back(samples[c].name);
        all_inputs.insert(all_inputs.end(), samples[c].inputs.begin(), samples[c].inputs.end());
        if (!opt.db_out.empty()) {
            outputs.push_back(opt.db_out + std::to_string(c) + ".kmc_pre");
            outputs.push_back(opt.db_out + std::to_string(c) + ".kmc_suf");
        }
    }
    if (!gfa_path.empty()) { outputs.push_back(gfa_path); outputs.push_back(col_path); }
    std::vector<std::vector<ReadsInput>> reads(C);   // what each input is, per sample: decided here, once, for both passes
    {
        std::vector<ReadsInput> all;
        if (fastq_preflight("run-multi", "read", all_inputs, outputs, ReadsOptions{opt.gz, opt.fasta}, all, err)) return 1;
        auto at = all.begin();
        for (uint32_t c = 0; c < C; at += (ptrdiff_t)samples[c++].inputs.size()) reads[c].assign(at, at + (ptrdiff_t)samples[c].inputs.size());
    }
    for (uint32_t c = 0; c < C; ++c)   // one file under two names
        for (uint32_t d = 0; d < c; ++d)
            for (const std::string &a : samples[c].inputs)
                for (const std::string &b : samples[d].inputs)
                    if (same_file(a, b)) {
                        err = "run-multi: " + a + ": the same file is given in two samples (" + samples[d].name + " as " + b + ", " + samples[c].name + ")";
                        return 1;
                    }

    pf_clip::Adapters adapters;   // --adapters: read and refused here, before a device context exists
    if (opt.trim.clip.on() && clip_load(opt.trim.clip, adapters, err)) { err = "run-multi: " + err; return 1; }

    pf_ctx *ctx = nullptr;
    if (pf_create(device, &ctx) != PF_OK) {
        err = std::string("run-multi: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); reads are counted and called on the GPU only";
        return 1;
    }
    // (the context goes to the CCDBG in the end: destroyed here only on the way out before that)
    CtxGuard ctx_guard{ctx};
    DeviceArrays held(ctx_guard.c);
    std::vector<std::string> db_tmp;   // prefixes of the databases written so far, under their temporary names
    bool gfa_tmp_written = false;
    auto fail = [&](const std::string &m) {   // nothing is left under any output name after a refusal
        err = m;
        for (const std::string &p : db_tmp) { unlink((p + ".kmc_pre").c_str()); unlink((p + ".kmc_suf").c_str()); }
        if (gfa_tmp_written) { unlink(gfa_tmp.c_str()); unlink(col_tmp.c_str()); }
        return 1;
    };
    auto dev_fail = [&]() { return fail(std::string("run-multi: ") + pf_last_error(ctx)); };

    std::vector<std::vector<ClipCounts>> unit_clip(C);
    if (opt.trim.clip.on()) {   // the clip stays open over both passes; the first one is reported
        if (clip_open(ctx, adapters, opt.trim.clip) != PF_OK) return dev_fail();
        for (uint32_t c = 0; c < C; ++c) unit_clip[c].assign(trim_unit_count(samples[c].inputs.size(), samples[c].paired), ClipCounts{});
    }
    if (opt.trim.dedup.on) {   // a fresh table per unit in both passes; the first one is reported
        stats.dedup.resize(C);
        for (uint32_t c = 0; c < C; ++c) stats.dedup[c].assign(trim_unit_count(samples[c].inputs.size(), samples[c].paired), pf_dedup_stats{});
    }
    // ---- first pass, per sample: count, thresholds; the counters stay resident ----
    stats.colors = C;
    stats.color.assign(C, RunMultiColor{});
    if (trimming) {
        stats.trim.resize(C);
        for (uint32_t c = 0; c < C; ++c) stats.trim[c].assign(samples[c].paired ? samples[c].inputs.size() : 1, pf_trim_stats{});
    }
    std::vector<Counted> db(C), kept(C);
    std::vector<std::vector<uint64_t>> rows(C);
    for (uint32_t c = 0; c < C; ++c) {
        const auto t_count = clk::now();
        pf_count_stats counted = {};
        CountTimes ctm;
        std::string e;
        if (trimming ? count_stream_with(ctx, "run-multi", copt, [&](std::string &pe) {
                           return stream_trimmed(ctx, "run-multi", reads[c], samples[c].paired, opt.trim, opt.chunk_bytes, false, 0, 0, stats.trim[c].data(),
                                                 nullptr, pe, unit_clip[c].empty() ? nullptr : unit_clip[c].data(),
                                                 stats.dedup.empty() ? nullptr : stats.dedup[c].data());
                       }, db[c], counted, ctm, e)
                     : count_stream(ctx, "run-multi", reads[c], copt, db[c], counted, ctm, e))
            return fail(e);
        held.p.push_back(db[c].kmers);
        held.p.push_back(db[c].counts);
        stats.reads += counted.reads;
        stats.bases += counted.bases;
        stats.kmers += counted.kmers;
        stats.bad += counted.kmers_bad;
        stats.distinct += counted.unique;
        stats.color[c].distinct = db[c].n;
        if (counted_rows(ctx, db[c], copt, rows[c]) != PF_OK) return fail(std::string("run-multi: histogram of the counters of sample ") + samples[c].name + ": " + pf_last_error(ctx));
        int lo = 0, hi = 0;
        if (cutoffs_from_rows(rows[c], opt.quantile, lo, hi)) return fail("Error: Histogram File is badly Formatted.");
        lo = std::max(10, lo);
        stats.color[c].lower = (uint32_t)lo;
        stats.color[c].upper = (uint32_t)std::max(hi, 0);
        if (stats.color[c].lower > opt.mask_up)
            return fail("run-multi: the derived lower threshold " + std::to_string(lo) + " of sample " + samples[c].name + " is above the upper threshold " +
                        std::to_string(opt.mask_up));
        printf("%u\n", stats.color[c].lower);   // exactly as `mask --auto-cutoffs` prints it
        fflush(stdout);
        tm.count_s += since(t_count);
        if (!opt.db_out.empty()) {
            const auto t_db = clk::now();
            const std::string p = opt.db_out + std::to_string(c) + tail;
            db_tmp.push_back(p);
            if (write_counted(ctx, "run-multi", p, db[c], copt, e)) return fail(e);
            tm.db_out_s += since(t_db);
        }
    }

    // ---- second pass, per sample: the k-mers of its masked reads, without the masked reads ----
    for (uint32_t c = 0; c < C; ++c) {
        const auto t_stream = clk::now();
        if (pf_upload_counts(ctx, db[c].kmers, db[c].counts, db[c].n, opt.k, opt.ci, opt.cx, 1) != PF_OK)
            return fail(std::string("run-multi: count table of sample ") + samples[c].name + ": " + pf_last_error(ctx));
        if (pf_count_begin(ctx, opt.k, 1, opt.initial_slots) != PF_OK) return dev_fail();
        StreamTimes stm;
        std::string e;
        pf_maskcount_stats masked = {};
        if (trimming ? stream_trimmed(ctx, "run-multi", reads[c], samples[c].paired, opt.trim, opt.chunk_bytes, true, stats.color[c].lower, opt.mask_up, nullptr,
                                      &masked, e)
                     : stream_fastq(ctx, "run-multi", reads[c], opt.chunk_bytes, -1, "",
                         [&](const Chunk &ch, Taken &t) {
                             pf_maskcount_stats st = {};
                             const int rc = ch.fasta ? pf_maskcount_fasta(ctx, ch.text, ch.n, ch.final ? 1 : 0, stats.color[c].lower, opt.mask_up, &t.used, &st, &t.bad)
                                                     : pf_maskcount_fastq(ctx, ch.text, ch.n, ch.final ? 1 : 0, stats.color[c].lower, opt.mask_up, &t.used, &st, &t.bad);
                             if (rc != PF_OK) return rc;
                             t.reads = st.reads;
                             stats.windows_bad += st.kmers_bad;
                             stats.windows_kept += st.kmers_kept;
                             return (int)PF_OK;
                         },
                         stm, e)) {
            pf_count_abort(ctx);
            return fail(e);
        }
        stats.windows_bad += masked.kmers_bad;
        stats.windows_kept += masked.kmers_kept;
        pf_count_stats st2 = {};
        if (pf_count_finish(ctx, 1, pf_count::COUNTER_MAX, pf_count::COUNTER_MAX, &kept[c].kmers, &kept[c].counts, &kept[c].n, &st2) != PF_OK) {
            const int rc = dev_fail();
            pf_count_abort(ctx);
            return rc;
        }
        pf_device_free(ctx, kept[c].counts);   // union and colouring ask for the k-mers alone
        kept[c].counts = nullptr;
        held.p.push_back(kept[c].kmers);
        stats.color[c].kept = kept[c].n;
        tm.recount_s += since(t_stream);
    }
    if (opt.trim.clip.on()) {
        stats.clip.resize(C);
        for (uint32_t c = 0; c < C; ++c)
            for (const ClipCounts &u : unit_clip[c]) stats.clip[c].push_back(clip_report_of(adapters, opt.trim.clip, u));
        if (pf_clip_end(ctx) != PF_OK) return dev_fail();
    }
    if (pf_release_counts(ctx) != PF_OK) return dev_fail();   // the last sample's table: the joined one takes its place in the end

    // ---- union: the vertices ----
    const auto t_union = clk::now();
    uint64_t *verts = nullptr, n_verts = 0;
    {
        std::vector<const uint64_t *> sets(C);
        std::vector<uint64_t> ns(C);
        for (uint32_t c = 0; c < C; ++c) { sets[c] = kept[c].kmers; ns[c] = kept[c].n; }
        if (pf_kmer_union(ctx, C, sets.data(), ns.data(), &verts, &n_verts) != PF_OK) return dev_fail();
        held.p.push_back(verts);
    }
    stats.distinct_kept = n_verts;
    tm.union_s = since(t_union);
    if (n_verts == 0) return fail("ColoredCDBG::read(): Graph could not be loaded! Exit. (no k-mer of any sample survives the masking)");
    if (n_verts >= pf_unitig::MAX_KMERS) return fail(std::string("run-multi: ") + pf_unitig::TOO_MANY_TEXT + " (" + std::to_string(n_verts) + ")");

    // ---- graph, with the colour sets placed ----
    const auto t_graph = clk::now();
    const uint32_t g = opt.g == BuildOptions::G_DEFAULT ? PF_UNITIG_G_DEFAULT : (uint32_t)opt.g;
    if (pf_unitig_build_colored(ctx, verts, n_verts, opt.k, g, opt.clip_tips ? 1 : 0, opt.del_isolated ? 1 : 0, n_seeds, &stats.graph, &stats.overflow) != PF_OK)
        return dev_fail();
    tm.graph_s = since(t_graph);

    // ---- colours: one look-up per distinct k-mer of every sample ----
    const auto t_color = clk::now();
    if (pf_color_begin(ctx, C) != PF_OK) return dev_fail();
    held.drop(verts, ctx);   // the table holds the keys from here
    for (uint32_t c = 0; c < C; ++c) {
        pf_color_kmers_stats ks = {};
        if (pf_color_kmers(ctx, c, kept[c].kmers, kept[c].n, &ks) != PF_OK) return dev_fail();
        stats.kmers_colored += ks.kmers_colored;
        stats.kmers_unplaced += ks.kmers_unplaced;
        held.drop(kept[c].kmers, ctx);
        kept[c].kmers = nullptr;
    }
    pf_color_stats colored = {};
    if (pf_color_finish(ctx, &colored) != PF_OK) return dev_fail();
    stats.runs = colored.runs;
    tm.color_s = since(t_color);

    // ---- serialise: runs and slots into the bytes of the colour file ----
    const auto t_ser = clk::now();
    std::vector<uint8_t> col_bytes;
    {
        pf_color::Colored cg;
        const uint64_t nl = colored.lines;
        std::vector<uint64_t> heads((size_t)nl);
        std::vector<uint32_t> m((size_t)nl), slot((size_t)nl);
        cg.run_off.resize((size_t)nl + 1);
        cg.runs.resize((size_t)colored.runs);
        static_assert(sizeof(pf_color::Run) == 8, "a run is two 32-bit words, as the device writes them");
        if (pf_color_fetch(ctx, heads.data(), m.data(), slot.data(), cg.run_off.data(), reinterpret_cast<uint32_t *>(cg.runs.data())) != PF_OK) return dev_fail();
        cg.lines.resize((size_t)nl);
        for (uint64_t j = 0; j < nl; ++j) {
            cg.lines[j].head = heads[j];
            cg.lines[j].m = m[j];
            cg.lines[j].slot = slot[j];
        }
        cg.overflow = stats.overflow;
        const std::string why = pf_bfg::write(cg, (int)opt.k, n_seeds, names, col_bytes);
        if (!why.empty()) return fail("run-multi: " + why);
    }
    stats.color_bytes = col_bytes.size();
    tm.serialise_s = since(t_ser);

    // ---- hand-off: the text stays where it is; the host gets its one copy (the size of the graph, not of the reads) ----
    const auto t_load = clk::now();
    const char *dev_text = nullptr;
    uint64_t n_text = 0;
    if (pf_unitig_text(ctx, &dev_text, &n_text) != PF_OK) return dev_fail();
    std::vector<char> host_text((size_t)n_text);
    if (pf_unitig_fetch(ctx, 0, n_text, host_text.data()) != PF_OK) return dev_fail();
    if (!gfa_path.empty()) {
        const auto t_gfa = clk::now();
        std::string why;
        gfa_tmp_written = true;
        if (!write_file(gfa_tmp, host_text.data(), n_text, why) || !write_file(col_tmp, col_bytes.data(), col_bytes.size(), why)) return fail("run-multi: " + why);
        tm.gfa_out_s = since(t_gfa);
    }
    ColoredUnitigSet cset;
    if (!cset.open_memory(host_text.data(), n_text, dev_text, col_bytes.data(), col_bytes.size(), mopt.call.threads))
        return fail("ColoredCDBG::read(): Graph could not be loaded! Exit. (" + cset.err + ")");
    ColorCounts counts;
    counts.ctx = ctx;
    counts.k = (int)opt.k;
    counts.min_count = opt.ci;
    counts.max_count = opt.cx;
    for (uint32_t c = 0; c < C; ++c) {
        counts.kmers.push_back(db[c].kmers);
        counts.counts.push_back(db[c].counts);
        counts.n.push_back(db[c].n);
    }
    ctx_guard.c = nullptr;   // the CCDBG's from here
    double match = opt.match, mismatch = opt.mismatch, gap = opt.gap;
    const size_t complex_size = opt.complex_size;
    CCDBG ccdbg(cset, complex_size, match, mismatch, gap, counts, device, false);
    for (uint32_t c = 0; c < C; ++c) {   // the joined table holds them (or the run ends here)
        pf_device_free(ccdbg.device(), db[c].kmers);
        pf_device_free(ccdbg.device(), db[c].counts);
    }
    if (!ccdbg.good()) {
        const std::string &e = ccdbg.error();
        const std::string plain = "CompactedDBG::read()";   // the coloured front end's words for the same refusal
        return fail(e.rfind(plain, 0) == 0 ? "ColoredCDBG::read()" + e.substr(plain.size()) : e);
    }
    tm.load_s = since(t_load) - tm.gfa_out_s;

    // ---- calling: the coloured path as the command line sets it up ----
    const auto t_call = clk::now();
    ColoredCallSetup call = mopt.call;
    call.outprefix = out_prefix;
    call.graphfile.clear();
    call.cutoffs.assign(C, std::pair<int, int>(10, 1000));
    call.color_rows = &rows;
    call.quantile = opt.quantile;
    {
        std::string e;
        if (colored_call_run(ccdbg, call, e)) return fail(e);
    }
    stats.model_last_line = ccdbg.model_last_line();
    tm.call_s = since(t_call);
    // ---- the optional outputs take their names ----
    for (uint32_t c = 0; c < (uint32_t)db_tmp.size(); ++c) {
        const std::string to = opt.db_out + std::to_string(c);
        for (const char *ext : {".kmc_suf", ".kmc_pre"})
            if (rename((db_tmp[c] + ext).c_str(), (to + ext).c_str()) != 0) {
                const int e = errno;
                for (uint32_t d = 0; d <= c; ++d) { unlink((opt.db_out + std::to_string(d) + ".kmc_suf").c_str()); unlink((opt.db_out + std::to_string(d) + ".kmc_pre").c_str()); }
                return fail("run-multi: renaming " + db_tmp[c] + ext + " to " + to + ext + " (" + strerror(e) + ")");
            }
    }
    if (!gfa_path.empty()) {
        if (rename(gfa_tmp.c_str(), gfa_path.c_str()) != 0) return fail("run-multi: renaming " + gfa_tmp + " to " + gfa_path + " (" + strerror(errno) + ")");
        if (rename(col_tmp.c_str(), col_path.c_str()) != 0) {
            const int e = errno;
            unlink(gfa_path.c_str());
            return fail("run-multi: renaming " + col_tmp + " to " + col_path + " (" + strerror(e) + ")");
        }
    }
    fflush(stdout);
    if (times) *times = tm;
    return 0;
}

}  // namespace pfh
