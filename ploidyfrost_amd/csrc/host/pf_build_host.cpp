#include "pf_build_host.hpp"

#include "pf_bfg_write.hpp"
#include "pf_host_util.hpp"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>

namespace pfh {

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

constexpr uint64_t FETCH_BLOCK_BYTES = 64ull << 20;   // text a download

}  // namespace

std::string build_options_refusal(const BuildOptions &opt) {
    if (!pf_count::k_ok(opt.k)) return pf_count::cut_text(pf_count::CUT_K);
    if (opt.g != BuildOptions::G_DEFAULT && !pf_unitig::g_ok(opt.g, (int)opt.k)) return pf_unitig::g_text((int)opt.k);
    return "";
}

int build_fastq(const std::vector<std::string> &inputs, const std::string &out_prefix, const BuildOptions &opt, int device, pf_count_stats &counted,
                pf_unitig_stats &stats, BuildTimes *times, std::string &err) {
    counted = pf_count_stats{};
    stats = pf_unitig_stats{};
    BuildTimes tm;
    // ---- refusals that need no device ----
    if (inputs.empty()) { err = "build: no input"; return 1; }
    if (out_prefix.empty()) { err = "build: no output prefix"; return 1; }
    { const std::string why = build_options_refusal(opt); if (!why.empty()) { err = "build: " + why; return 1; } }
    const std::string out_path = out_prefix + ".gfa";
    std::vector<ReadsInput> reads;
    if (fastq_preflight("build", "read", inputs, {out_path}, ReadsOptions{0, opt.fasta}, reads, err)) return 1;

    pf_ctx *ctx = nullptr;
    if (pf_create(device, &ctx) != PF_OK) {
        err = std::string("build: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); the graph is built on the GPU only";
        return 1;
    }
    CtxGuard ctx_guard{ctx};
    // ---- count: every k-mer of the reads, both strands ----
    CountOptions copt;
    copt.k = opt.k;
    copt.ci = 1;
    copt.cx = pf_count::COUNTER_MAX;
    copt.cs = pf_count::COUNTER_MAX;
    copt.both_strands = true;
    copt.chunk_bytes = opt.chunk_bytes;
    copt.initial_slots = opt.initial_slots;
    Counted db;
    CountTimes ctm;
    if (count_stream(ctx, "build", reads, copt, db, counted, ctm, err)) return 1;
    struct Free { pf_ctx *c; Counted &d; ~Free() { pf_device_free(c, d.kmers); pf_device_free(c, d.counts); } } free_db{ctx, db};
    tm.stream_s = ctm.stream_s;
    tm.finish_s = ctm.finish_s;
    pf_device_free(ctx, db.counts);   // the graph asks for the k-mers alone
    db.counts = nullptr;
    if (db.n >= pf_unitig::MAX_KMERS) { err = std::string("build: ") + pf_unitig::TOO_MANY_TEXT + " (" + std::to_string(db.n) + ")"; return 1; }
    // ---- graph ----
    const auto t_graph = clk::now();
    const uint32_t g = opt.g == BuildOptions::G_DEFAULT ? PF_UNITIG_G_DEFAULT : (uint32_t)opt.g;
    if (pf_unitig_build(ctx, db.kmers, db.n, opt.k, g, opt.clip_tips ? 1 : 0, opt.del_isolated ? 1 : 0, &stats) != PF_OK) {
        err = std::string("build: ") + pf_last_error(ctx);
        return 1;
    }
    tm.graph_s = since(t_graph);
    // ---- write: block by block through a pinned buffer ----
    const auto t_write = clk::now();
    const std::string tmp = out_path + ".tmp." + std::to_string((long)getpid());
    auto fail = [&](const std::string &m) {
        err = m;
        unlink(tmp.c_str());
        return 1;
    };
    const uint64_t block = std::max<uint64_t>(1, std::min<uint64_t>(stats.bytes, FETCH_BLOCK_BYTES));
    ChunkBuf buf;
    if (!buf.alloc(ctx, (size_t)block)) return fail("build: no memory for the text buffer");
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail("build: cannot write " + tmp + " (" + strerror(errno) + ")");
    for (uint64_t at = 0; at < stats.bytes; at += block) {
        const uint64_t nb = std::min<uint64_t>(block, stats.bytes - at);
        if (pf_unitig_fetch(ctx, at, nb, buf.p) != PF_OK) { close(fd); return fail(std::string("build: ") + pf_last_error(ctx)); }
        if (!write_all(fd, buf.p, nb)) { const int e = errno; close(fd); return fail("build: writing " + tmp + " (" + strerror(e) + ")"); }
    }
    if (close(fd) != 0) return fail("build: closing " + tmp + " (" + strerror(errno) + ")");
    if (rename(tmp.c_str(), out_path.c_str()) != 0) return fail("build: renaming " + tmp + " to " + out_path + " (" + strerror(errno) + ")");
    pf_unitig_release(ctx);
    tm.write_s = since(t_write);
    if (times) *times = tm;
    return 0;
}

std::string colored_inputs_refusal(const std::vector<std::string> &inputs) {
    if (inputs.size() > pf_color::MAX_COLORS) return std::string(pf_color::TOO_MANY_COLORS_TEXT) + ": " + std::to_string(inputs.size());
    for (size_t i = 0; i < inputs.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if (inputs[i] == inputs[j] || same_file(inputs[i], inputs[j]))
                return inputs[i] + ": the same file is given twice (-r " + std::to_string(j + 1) + " and -r " + std::to_string(i + 1) + "): a colour is a file";
    return "";
}

int build_colored_fastq(const std::vector<std::string> &inputs, const std::string &out_prefix, const BuildOptions &opt, uint32_t n_seeds, int device,
                        pf_count_stats &counted, pf_unitig_stats &stats, pf_color_stats &colored, uint64_t &color_bytes, ColoredTimes *times,
                        std::string &err) {
    counted = pf_count_stats{};
    stats = pf_unitig_stats{};
    colored = pf_color_stats{};
    color_bytes = 0;
    ColoredTimes tm;
    if (n_seeds == 0) n_seeds = pf_color::DEFAULT_SEEDS;
    // ---- refusals that need no device ----
    if (inputs.empty()) { err = "build-multi: no input"; return 1; }
    if (out_prefix.empty()) { err = "build-multi: no output prefix"; return 1; }
    { const std::string why = build_options_refusal(opt); if (!why.empty()) { err = "build-multi: " + why; return 1; } }
    if (!pf_color::seeds_ok(n_seeds)) { err = "build-multi: " + pf_color::seeds_text(); return 1; }
    { const std::string why = colored_inputs_refusal(inputs); if (!why.empty()) { err = "build-multi: " + why; return 1; } }
    const std::string gfa_path = out_prefix + ".gfa", col_path = out_prefix + ".bfg_colors";
    std::vector<ReadsInput> reads;
    if (fastq_preflight("build-multi", "read", inputs, {gfa_path, col_path}, ReadsOptions{0, opt.fasta}, reads, err)) return 1;

    pf_ctx *ctx = nullptr;
    if (pf_create(device, &ctx) != PF_OK) {
        err = std::string("build-multi: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); the graph is built on the GPU only";
        return 1;
    }
    CtxGuard ctx_guard{ctx};
    auto dev_fail = [&]() { err = std::string("build-multi: ") + pf_last_error(ctx); return 1; };
    // ---- count: every k-mer of all files, both strands ----
    CountOptions copt;
    copt.k = opt.k;
    copt.ci = 1;
    copt.cx = pf_count::COUNTER_MAX;
    copt.cs = pf_count::COUNTER_MAX;
    copt.both_strands = true;
    copt.chunk_bytes = opt.chunk_bytes;
    copt.initial_slots = opt.initial_slots;
    Counted db;
    CountTimes ctm;
    if (count_stream(ctx, "build-multi", reads, copt, db, counted, ctm, err)) return 1;
    struct Free { pf_ctx *c; Counted &d; ~Free() { pf_device_free(c, d.kmers); pf_device_free(c, d.counts); } } free_db{ctx, db};
    tm.build.stream_s = ctm.stream_s;
    tm.build.finish_s = ctm.finish_s;
    pf_device_free(ctx, db.counts);
    db.counts = nullptr;
    if (db.n >= pf_unitig::MAX_KMERS) { err = std::string("build-multi: ") + pf_unitig::TOO_MANY_TEXT + " (" + std::to_string(db.n) + ")"; return 1; }
    // ---- graph, with the colour sets placed ----
    const auto t_graph = clk::now();
    const uint32_t g = opt.g == BuildOptions::G_DEFAULT ? PF_UNITIG_G_DEFAULT : (uint32_t)opt.g;
    uint64_t overflow = 0;
    if (pf_unitig_build_colored(ctx, db.kmers, db.n, opt.k, g, opt.clip_tips ? 1 : 0, opt.del_isolated ? 1 : 0, n_seeds, &stats, &overflow) != PF_OK) return dev_fail();
    struct Release { pf_ctx *c; ~Release() { pf_unitig_release(c); } } release{ctx};
    tm.build.graph_s = since(t_graph);
    // ---- colour: every file once more ----
    const auto t_color = clk::now();
    if (pf_color_begin(ctx, (uint32_t)inputs.size()) != PF_OK) return dev_fail();
    pf_device_free(ctx, db.kmers);   // the table holds the keys from here
    db.kmers = nullptr;
    for (size_t c = 0; c < inputs.size(); ++c) {
        StreamTimes stm;
        if (stream_fastq(ctx, "build-multi", {reads[c]}, opt.chunk_bytes, -1, "",
                         [&](const Chunk &ch, Taken &t) {
                             pf_color_stats st = {};
                             const int rc = ch.fasta ? pf_color_fasta(ctx, (uint32_t)c, ch.text, ch.n, ch.final ? 1 : 0, &t.used, &st, &t.bad)
                                                     : pf_color_fastq(ctx, (uint32_t)c, ch.text, ch.n, ch.final ? 1 : 0, &t.used, &st, &t.bad);
                             t.reads = st.reads;
                             return rc;
                         },
                         stm, err))
            return 1;
    }
    if (pf_color_finish(ctx, &colored) != PF_OK) return dev_fail();
    tm.color_s = since(t_color);
    // ---- serialise: runs and slots into the bytes of the colour file ----
    const auto t_ser = clk::now();
    pf_color::Colored cg;
    std::vector<uint8_t> col_bytes;
    {
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
        cg.overflow = overflow;
        const std::string why = pf_bfg::write(cg, (int)opt.k, n_seeds, inputs, col_bytes);
        if (!why.empty()) { err = "build-multi: " + why; return 1; }
    }
    color_bytes = col_bytes.size();
    tm.serialise_s = since(t_ser);
    // ---- write: the text block by block through a pinned buffer, then the colour file; both renamed at the end ----
    const auto t_write = clk::now();
    const std::string tail = ".tmp." + std::to_string((long)getpid());
    const std::string gfa_tmp = gfa_path + tail, col_tmp = col_path + tail;
    auto fail = [&](const std::string &m) {
        err = m;
        unlink(gfa_tmp.c_str());
        unlink(col_tmp.c_str());
        return 1;
    };
    const uint64_t block = std::max<uint64_t>(1, std::min<uint64_t>(stats.bytes, FETCH_BLOCK_BYTES));
    ChunkBuf buf;
    if (!buf.alloc(ctx, (size_t)block)) return fail("build-multi: no memory for the text buffer");
    int fd = open(gfa_tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail("build-multi: cannot write " + gfa_tmp + " (" + strerror(errno) + ")");
    for (uint64_t at = 0; at < stats.bytes; at += block) {
        const uint64_t nb = std::min<uint64_t>(block, stats.bytes - at);
        if (pf_unitig_fetch(ctx, at, nb, buf.p) != PF_OK) { close(fd); return fail(std::string("build-multi: ") + pf_last_error(ctx)); }
        if (!write_all(fd, buf.p, nb)) { const int e = errno; close(fd); return fail("build-multi: writing " + gfa_tmp + " (" + strerror(e) + ")"); }
    }
    if (close(fd) != 0) return fail("build-multi: closing " + gfa_tmp + " (" + strerror(errno) + ")");
    fd = open(col_tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail("build-multi: cannot write " + col_tmp + " (" + strerror(errno) + ")");
    if (!write_all(fd, col_bytes.data(), col_bytes.size())) { const int e = errno; close(fd); return fail("build-multi: writing " + col_tmp + " (" + strerror(e) + ")"); }
    if (close(fd) != 0) return fail("build-multi: closing " + col_tmp + " (" + strerror(errno) + ")");
    if (rename(gfa_tmp.c_str(), gfa_path.c_str()) != 0) return fail("build-multi: renaming " + gfa_tmp + " to " + gfa_path + " (" + strerror(errno) + ")");
    if (rename(col_tmp.c_str(), col_path.c_str()) != 0) {
        const int e = errno;
        unlink(gfa_path.c_str());
        return fail("build-multi: renaming " + col_tmp + " to " + col_path + " (" + strerror(e) + ")");
    }
    tm.build.write_s = since(t_write);
    if (times) *times = tm;
    return 0;
}

}  // namespace pfh
