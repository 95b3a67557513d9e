#include "pf_qc_host.hpp"

#include "../pf_trim_rule.hpp"
#include "pf_host_util.hpp"
#include "pf_reads_stream.hpp"

namespace pfh {

int qc_fastq(const std::vector<std::string> &inputs1, const std::vector<std::string> &inputs2, const std::string &report_path, const QcOptions &opt,
             int device, QcReport &report, std::string &err) {
    report = QcReport{};
    err.clear();
    // ---- refusals that need no device ----
    if (inputs1.empty() && inputs2.empty()) { err = "qc: no input"; return 1; }
    if (report_path.empty()) { err = "qc: no report path"; return 1; }
    if (opt.phred != 33 && opt.phred != 64) { err = std::string("qc: ") + pf_trim::refusal_text(pf_trim::REFUSE_PHRED) + ", not " + std::to_string(opt.phred); return 1; }
    std::vector<std::string> inputs = inputs1;
    inputs.insert(inputs.end(), inputs2.begin(), inputs2.end());
    std::vector<ReadsInput> reads;
    if (fastq_preflight("qc", "reported", inputs, {report_path}, ReadsOptions{opt.gz, false}, reads, err)) return 1;
    pf_ctx *ctx = nullptr;
    if (pf_create(device, &ctx) != PF_OK) {
        err = std::string("qc: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); reads are reported on the GPU only";
        return 1;
    }
    CtxGuard ctx_guard{ctx};
    if (qc_open(ctx, opt.phred, "qc", err)) return 1;
    OutFiles outs("qc");
    if (outs.open_all({report_path}, err)) return 1;
    for (size_t i = 0; i < reads.size(); ++i) {   // each file on its own: a file's last record ends with the file
        const int side = i < inputs1.size() ? 0 : 1;
        StreamTimes tm;
        if (stream_fastq(ctx, "qc", std::vector<ReadsInput>{reads[i]}, opt.chunk_bytes, -1, "",
                         [&](const Chunk &c, Taken &t) { return pf_qc_fastq(ctx, side, c.text, c.n, c.final ? 1 : 0, &t.used, &t.reads, &t.bad); }, tm, err))
            return 1;
    }
    if (qc_close(ctx, opt.phred, false, "qc", report, err)) return 1;
    const std::string text = report.text();
    if (!write_all(outs.f[0].fd, text.data(), text.size(), "qc", outs.f[0].tmp, err)) return 1;
    return outs.commit(err);
}

}  // namespace pfh
