#include "pf_trim_host.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <thread>

#include "../pf_trim_rule.hpp"
#include "pf_host_util.hpp"
#include "pf_gz_out_host.hpp"
#include "pf_reads_stream.hpp"

static_assert(sizeof(pf_trim_step) == sizeof(pf_trim::Step) && sizeof(pf_trim_stats) == sizeof(pf_trim::Stats), "the rule header restates the ABI's records");

namespace pfh {

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

// Trimmomatic's five columns for record r of a chunk whose lines are (lb, le)
// (n: the bases of the read, or with --adapters its clip end -- the log speaks of the read the steps saw)
void trimlog_line(std::string &log, const char *text, const uint64_t *lb, const uint64_t *le, uint32_t begin, uint32_t len, const uint32_t *clip_end = nullptr) {
    log.append(text + lb[0] + 1, le[0] - lb[0] - 1);   // (the header starts with '@': the index has checked it)
    if (!len) { log += " 0 0 0 0\n"; return; }
    const uint64_t n = clip_end ? (uint64_t)*clip_end : le[3] - lb[3], e = (uint64_t)begin + len;
    log += ' ' + std::to_string(len) + ' ' + std::to_string(begin) + ' ' + std::to_string(e) + ' ' + std::to_string(n - e) + '\n';
}

// everything that is refused before a device context exists
int trim_preflight(const std::vector<std::string> &inputs, const std::vector<std::string> &outputs, const TrimOptions &opt, std::vector<ReadsInput> &reads,
                   pf_clip::Adapters &adapters, std::string &err) {
    if (trim_options_clause(opt, err)) return 1;
    if (opt.clip.on() && clip_load(opt.clip, adapters, err)) { err = "trim: " + err; return 1; }
    for (size_t i = 0; i < outputs.size(); ++i) {
        if (outputs[i].empty()) { err = "trim: an output path is empty"; return 1; }
        for (size_t j = 0; j < i; ++j)
            if (same_file(outputs[i], outputs[j])) { err = "trim: two outputs have the same path (" + outputs[i] + ")"; return 1; }
    }
    return fastq_preflight("trim", "trimmed", inputs, outputs, ReadsOptions{opt.gz, false}, reads, err);
}

int trim_create(int device, pf_ctx **ctx, std::string &err) {
    if (pf_create(device, ctx) == PF_OK) return 0;
    err = std::string("trim: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); reads are trimmed on the GPU only";
    return 1;
}
// --adapters: the clip of the whole stream, opened on the fresh context (it goes with the context)
int trim_clip_open(pf_ctx *ctx, const TrimOptions &opt, const pf_clip::Adapters &adapters, std::string &err) {
    if (!opt.clip.on() || clip_open(ctx, adapters, opt.clip) == PF_OK) return 0;
    err = std::string("trim: ") + pf_last_error(ctx);
    return 1;
}
// --report: the report opened on the fresh context; closed, worded and written into its output file when the stream has ended
int trim_qc_open(pf_ctx *ctx, const TrimOptions &opt, std::string &err) { return opt.report.empty() ? 0 : qc_open(ctx, opt.phred, "trim", err); }
int trim_qc_write(pf_ctx *ctx, const TrimOptions &opt, const OutFiles::File &f, QcReport *qc, std::string &err) {
    if (opt.report.empty()) return 0;
    QcReport r;
    if (qc_close(ctx, opt.phred, opt.clip.on(), "trim", r, err)) return 1;
    const std::string text = r.text();
    if (!write_all(f.fd, text.data(), text.size(), "trim", f.tmp, err)) return 1;
    if (qc) *qc = std::move(r);
    return 0;
}
// --dedup: the table of the whole stream, opened on the fresh context; its statistics when the stream has ended
int trim_dedup_open(pf_ctx *ctx, const TrimOptions &opt, std::string &err) {
    if (dedup_open(ctx, opt.dedup) == PF_OK) return 0;
    err = std::string("trim: ") + pf_last_error(ctx);
    return 1;
}
int trim_dedup_report(pf_ctx *ctx, const TrimOptions &opt, pf_dedup_stats *dedup, std::string &err) {
    if (dedup_close(ctx, opt.dedup, dedup) == PF_OK) return 0;
    err = std::string("trim: ") + pf_last_error(ctx);
    return 1;
}
int trim_clip_report(pf_ctx *ctx, const TrimOptions &opt, const pf_clip::Adapters &adapters, ClipReport *clip, std::string &err) {
    if (!opt.clip.on() || !clip || clip_report(ctx, adapters, opt.clip, *clip) == PF_OK) return 0;
    err = std::string("trim: ") + pf_last_error(ctx);
    return 1;
}

}  // namespace

int trim_options_clause(const TrimOptions &opt, std::string &err) {
    uint32_t bad = 0;
    int c = pf_trim::steps_clause(reinterpret_cast<const pf_trim::Step *>(opt.steps.data()), (uint32_t)opt.steps.size(), opt.phred, &bad);
    if (c == pf_trim::REFUSE_NO_STEP && opt.clip.on() && opt.steps.empty()) c = 0;   // --adapters alone is a plan
    if (c == pf_trim::REFUSE_NO_STEP && opt.dedup.on && opt.steps.empty()) c = 0;    // and so is --dedup
    if (!c) {
        const std::string why = dedup_options_refusal(opt.dedup);
        if (!why.empty()) { err = "trim: " + why; return -1; }
    }
    if (!c && opt.clip.on()) {
        int cc = pf_clip::params_clause(opt.clip.seed, opt.clip.score);
        if (!cc && opt.clip.pairs) cc = pf_clip::pair_params_clause(opt.clip.pair_score, opt.clip.pair_min);
        if (cc) { err = std::string("trim: ") + pf_clip::refusal_text(cc); return cc; }
    }
    if (!c) return 0;
    err = std::string("trim: ") + pf_trim::refusal_text(c);
    if (c == pf_trim::REFUSE_PHRED) err += ", not " + std::to_string(opt.phred);
    else if (c != pf_trim::REFUSE_NO_STEP && c != pf_trim::REFUSE_TOO_MANY) err += " (step " + std::to_string(bad + 1) + ")";
    return c;
}

int trim_fastq(const std::vector<std::string> &inputs, const std::string &out_path, const TrimOptions &opt, int device, pf_trim_stats &stats,
               TrimTimes *times, std::string &err, ClipReport *clip, QcReport *qc, pf_dedup_stats *dedup) {
    stats = pf_trim_stats{};
    err.clear();
    if (opt.clip.on() && opt.clip.pairs) { err = "trim: --adapter-pairs needs -1 / -2"; return 1; }
    const bool logs = !opt.trimlog.empty();
    std::vector<std::string> paths = {out_path};
    if (logs) paths.push_back(opt.trimlog);
    if (!opt.report.empty()) paths.push_back(opt.report);   // (the last output)
    std::vector<ReadsInput> reads;
    pf_clip::Adapters adapters;
    if (trim_preflight(inputs, paths, opt, reads, adapters, err)) return 1;
    pf_ctx *ctx = nullptr;
    if (trim_create(device, &ctx, err)) return 1;
    CtxGuard ctx_guard{ctx};
    if (trim_clip_open(ctx, opt, adapters, err) || trim_qc_open(ctx, opt, err) || trim_dedup_open(ctx, opt, err)) return 1;
    const auto t_stream = clk::now();
    OutFiles outs("trim");
    if (outs.open_all(paths, err)) return 1;
    std::vector<uint32_t> rb, rl, ce;
    std::vector<uint64_t> lb, le;
    std::string log, log_err;
    std::vector<char> fetched;
    StreamTimes st_tm;
    std::unique_ptr<GzOutFile> gzo;   // --gz-out: the output stays on the device until it is deflated, and the stream writes nothing itself
    if (opt.gz_out) {
        gzo.reset(new GzOutFile(ctx));
        gzo->start(outs.f[0].fd, "trim", outs.f[0].tmp);
    }
    stream_fastq(ctx, "trim", reads, opt.chunk_bytes, gzo ? -1 : outs.f[0].fd, outs.f[0].tmp,
                 [&](const Chunk &c, Taken &t) {
                     if (logs) { rb.resize(c.n / 4 + 1); rl.resize(c.n / 4 + 1); }
                     pf_trim_stats st = {};
                     char *out = c.out;
                     if (gzo && !(out = gzo->place(c.n + 1, err))) return (int)PF_ERR_HIP;   // (err is worded)
                     const int rc = pf_trim_fastq(ctx, c.text, c.n, c.final ? 1 : 0, opt.steps.data(), (uint32_t)opt.steps.size(), opt.phred, out, &t.out_len, &t.used,
                                                  logs ? rb.data() : nullptr, logs ? rl.data() : nullptr, &t.reads, &st, &t.bad);
                     if (rc != PF_OK) return rc;
                     if (gzo && !gzo->take(t.out_len, false, err)) return (int)PF_ERR_HIP;
                     add_trim_stats(stats, st);
                     if (logs && log_err.empty()) {   // on the host, from the (begin, len) arrays
                         const char *text = c.text;
                         if (c.on_device) {   // (inflated on the device: the log alone takes the text across)
                             fetched.resize(t.used);
                             if (t.used && pf_copy(ctx, fetched.data(), text, (size_t)t.used) != PF_OK) return (int)PF_ERR_HIP;
                             text = fetched.data();
                         }
                         pf_trim::record_lines(text, t.used, t.reads, lb, le);
                         if (opt.clip.on()) {
                             ce.resize(t.reads + 1);
                             if (pf_clip_last_ends(ctx, 0, ce.data(), t.reads) != PF_OK) return (int)PF_ERR_HIP;
                         }
                         log.clear();
                         for (uint64_t r = 0; r < t.reads; ++r) trimlog_line(log, text, &lb[4 * r], &le[4 * r], rb[r], rl[r], opt.clip.on() ? &ce[r] : nullptr);
                         write_all(outs.f[1].fd, log.data(), log.size(), "trim", outs.f[1].tmp, log_err);
                     }
                     return (int)PF_OK;
                 },
                 st_tm, err);
    if (gzo) {
        if (err.empty()) gzo->finish(err);
        gzo->stop();
        if (err.empty()) err = gzo->wr.err;
        st_tm.write_s = gzo->wr.write_s;
    }
    if (err.empty()) err = log_err;
    if (err.empty()) trim_clip_report(ctx, opt, adapters, clip, err);
    if (err.empty()) trim_dedup_report(ctx, opt, dedup, err);
    if (err.empty()) trim_qc_write(ctx, opt, outs.f.back(), qc, err);
    if (!err.empty() || outs.commit(err)) return 1;
    if (times) {
        times->stream_s = since(t_stream);
        times->device_s = st_tm.device_s;
        times->read_s = st_tm.read_s;
        times->write_s = st_tm.write_s;
    }
    return 0;
}

int trim_fastq_pair(const std::string &in1, const std::string &in2, const std::string out_paths[4], const TrimOptions &opt, int device,
                    pf_trim_stats stats[2], TrimTimes *times, std::string &err, ClipReport *clip, QcReport *qc, pf_dedup_stats *dedup) {
    stats[0] = stats[1] = pf_trim_stats{};
    err.clear();
    const bool logs = !opt.trimlog.empty();
    const std::vector<std::string> inputs = {in1, in2};
    std::vector<std::string> paths(out_paths, out_paths + 4);
    if (logs) paths.push_back(opt.trimlog);
    if (!opt.report.empty()) paths.push_back(opt.report);   // (the last output)
    std::vector<ReadsInput> reads;
    pf_clip::Adapters adapters;
    if (trim_preflight(inputs, paths, opt, reads, adapters, err)) return 1;
    if (same_file(in1, in2)) { err = "trim: the two inputs of a pair are the same file (" + in1 + ")"; return 1; }
    pf_ctx *ctx = nullptr;
    if (trim_create(device, &ctx, err)) return 1;
    CtxGuard ctx_guard{ctx};
    if (trim_clip_open(ctx, opt, adapters, err) || trim_qc_open(ctx, opt, err) || trim_dedup_open(ctx, opt, err)) return 1;
    const auto t_stream = clk::now();
    OutFiles outs("trim");
    if (outs.open_all(paths, err)) return 1;

    PieceWriter wr[4];
    std::unique_ptr<GzOutFile> gzo[4];   // --gz-out: the four outputs stay on the device until they are deflated
    for (int d = 0; d < 4; ++d) {
        if (opt.gz_out) {
            gzo[d].reset(new GzOutFile(ctx));
            gzo[d]->start(outs.f[d].fd, "trim", outs.f[d].tmp);
        } else {
            wr[d].start(outs.f[d].fd, "trim", outs.f[d].tmp);
        }
    }
    std::vector<uint32_t> rb[2], rl[2], ce[2];
    std::vector<uint64_t> lb[2], le[2];
    std::string log;
    std::vector<char> fetched[2];
    PairStreamTimes ptm;
    stream_fastq_pair(ctx, "trim", reads[0], reads[1], opt.chunk_bytes,
                      [&](const PairChunk &c, PairTaken &t) {
                          const char *text[2] = {c.text[0], c.text[1]};
                          std::shared_ptr<char> out[4];
                          char *out_p[4];
                          for (int d = 0; d < 4; ++d) {
                              if (opt.gz_out) {
                                  if (!(out_p[d] = gzo[d]->place(c.n[d / 2] + 1, err))) return (int)PF_ERR_HIP;   // (err is worded)
                                  continue;
                              }
                              out[d] = std::shared_ptr<char>(new char[c.n[d / 2] + 1], std::default_delete<char[]>());
                              out_p[d] = out[d].get();
                          }
                          uint32_t *rb_p[2] = {nullptr, nullptr}, *rl_p[2] = {nullptr, nullptr};
                          if (logs)
                              for (int f = 0; f < 2; ++f) {
                                  rb[f].resize(c.n[f] / 4 + 1);
                                  rl[f].resize(c.n[f] / 4 + 1);
                                  rb_p[f] = rb[f].data();
                                  rl_p[f] = rl[f].data();
                              }
                          uint64_t out_bytes[4] = {0, 0, 0, 0};
                          pf_trim_stats st[2] = {};
                          const int rc = pf_trim_fastq_pair(ctx, c.text[0], c.n[0], c.text[1], c.n[1], c.final ? 1 : 0, opt.steps.data(), (uint32_t)opt.steps.size(),
                                                            opt.phred, out_p, out_bytes, t.used, rb_p, rl_p, &t.reads, st, &t.bad);
                          if (rc != PF_OK) return rc;
                          add_trim_stats(stats[0], st[0]);
                          add_trim_stats(stats[1], st[1]);
                          if (logs) {
                              log.clear();
                              for (int f = 0; f < 2; ++f)
                                  if (c.on_device[f]) {   // (inflated on the device: the log alone takes the text across)
                                      fetched[f].resize(t.used[f]);
                                      if (t.used[f] && pf_copy(ctx, fetched[f].data(), text[f], (size_t)t.used[f]) != PF_OK) return (int)PF_ERR_HIP;
                                      text[f] = fetched[f].data();
                                  }
                              for (int f = 0; f < 2; ++f) pf_trim::record_lines(text[f], t.used[f], t.reads, lb[f], le[f]);
                              for (int f = 0; f < 2 && opt.clip.on(); ++f) {
                                  ce[f].resize(t.reads + 1);
                                  if (pf_clip_last_ends(ctx, f, ce[f].data(), t.reads) != PF_OK) return (int)PF_ERR_HIP;
                              }
                              for (uint64_t r = 0; r < t.reads; ++r)
                                  for (int f = 0; f < 2; ++f)
                                      trimlog_line(log, text[f], &lb[f][4 * r], &le[f][4 * r], rb[f][r], rl[f][r], opt.clip.on() ? &ce[f][r] : nullptr);
                              if (!write_all(outs.f[4].fd, log.data(), log.size(), "trim", outs.f[4].tmp, err)) return (int)PF_ERR_ARG;   // (err is worded)
                          }
                          for (int d = 0; d < 4; ++d) {
                              if (opt.gz_out) { if (!gzo[d]->take(out_bytes[d], false, err)) return (int)PF_ERR_HIP; }
                              else if (out_bytes[d]) wr[d].put(WritePiece{out[d], out_bytes[d]});
                          }
                          return (int)PF_OK;
                      },
                      ptm, err);
    for (int d = 0; d < 4; ++d) {
        if (!opt.gz_out) { wr[d].stop(); continue; }
        if (err.empty()) gzo[d]->finish(err);
        gzo[d]->stop();
    }
    for (int d = 0; d < 4 && err.empty(); ++d) err = opt.gz_out ? gzo[d]->wr.err : wr[d].err;
    if (err.empty()) trim_clip_report(ctx, opt, adapters, clip, err);
    if (err.empty()) trim_dedup_report(ctx, opt, dedup, err);
    if (err.empty()) trim_qc_write(ctx, opt, outs.f.back(), qc, err);
    if (!err.empty() || outs.commit(err)) return 1;
    if (times) {
        times->stream_s = since(t_stream);
        times->device_s = ptm.device_s;
        times->read_s = ptm.read_s;
        times->write_s = 0;
        for (int d = 0; d < 4; ++d) times->write_s += opt.gz_out ? gzo[d]->wr.write_s : wr[d].write_s;
    }
    return 0;
}

}  // namespace pfh
