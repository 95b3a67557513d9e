#include "pf_trim_host.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <memory>
#include <thread>

#include "../pf_trim_rule.hpp"
#include "pf_gz_host.hpp"
#include "pf_mask_host.hpp"

static_assert(sizeof(pf_trim_step) == sizeof(pf_trim::Step) && sizeof(pf_trim_stats) == sizeof(pf_trim::Stats), "the rule header restates the ABI's records");

namespace pfh {

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

// the outputs of a run: written under temporary names, renamed together at the end; nothing is left under any name otherwise
struct OutFiles {
    struct File { std::string path, tmp; int fd = -1; };
    std::vector<File> f;
    bool committed = false;
    int open_all(const std::vector<std::string> &paths, std::string &err) {
        for (const std::string &p : paths) {
            File o;
            o.path = p;
            o.tmp = p + ".tmp." + std::to_string((long)getpid());
            o.fd = open(o.tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            if (o.fd < 0) { err = "trim: cannot write " + o.tmp + " (" + strerror(errno) + ")"; return 1; }
            f.push_back(o);
        }
        return 0;
    }
    int commit(std::string &err) {
        for (File &o : f) {
            const int rc = close(o.fd);
            o.fd = -1;
            if (rc != 0 && err.empty()) err = "trim: closing " + o.tmp + " (" + strerror(errno) + ")";
        }
        for (size_t i = 0; i < f.size() && err.empty(); ++i)
            if (rename(f[i].tmp.c_str(), f[i].path.c_str()) != 0) {
                err = "trim: renaming " + f[i].tmp + " to " + f[i].path + " (" + strerror(errno) + ")";
                for (size_t j = 0; j < i; ++j) unlink(f[j].path.c_str());
            }
        committed = err.empty();
        return committed ? 0 : 1;
    }
    ~OutFiles() {
        if (committed) return;
        for (File &o : f) {
            if (o.fd >= 0) close(o.fd);
            unlink(o.tmp.c_str());
        }
    }
};

bool write_all(int fd, const char *p, uint64_t n, const std::string &name, std::string &err) {
    for (uint64_t done = 0; done < n;) {
        const ssize_t put = write(fd, p + done, (size_t)(n - done));
        if (put < 0 && errno == EINTR) continue;
        if (put < 0) { err = "trim: writing " + name + " (" + strerror(errno) + ")"; return false; }
        done += (uint64_t)put;
    }
    return true;
}

// Trimmomatic's five columns for record r of a chunk whose lines are (lb, le)
void trimlog_line(std::string &log, const char *text, const uint64_t *lb, const uint64_t *le, uint32_t begin, uint32_t len) {
    log.append(text + lb[0] + 1, le[0] - lb[0] - 1);   // (the header starts with '@': the index has checked it)
    if (!len) { log += " 0 0 0 0\n"; return; }
    const uint64_t n = le[3] - lb[3], e = (uint64_t)begin + len;
    log += ' ' + std::to_string(len) + ' ' + std::to_string(begin) + ' ' + std::to_string(e) + ' ' + std::to_string(n - e) + '\n';
}

void add_stats(pf_trim_stats &a, const pf_trim_stats &b) {
    a.reads += b.reads; a.kept += b.kept; a.dropped += b.dropped; a.bases += b.bases; a.bases_kept += b.bases_kept;
    a.both += b.both; a.only1 += b.only1; a.only2 += b.only2; a.neither += b.neither;
}

// everything that is refused before a device context exists
int trim_preflight(const std::vector<std::string> &inputs, const std::vector<std::string> &outputs, const TrimOptions &opt, uint64_t &largest,
                   std::string &err) {
    if (trim_options_clause(opt, err)) return 1;
    for (size_t i = 0; i < outputs.size(); ++i) {
        if (outputs[i].empty()) { err = "trim: an output path is empty"; return 1; }
        for (size_t j = 0; j < i; ++j)
            if (same_file(outputs[i], outputs[j])) { err = "trim: two outputs have the same path (" + outputs[i] + ")"; return 1; }
    }
    return fastq_preflight("trim", "trimmed", inputs, outputs, largest, err, opt.gz);
}

int trim_create(int device, pf_ctx **ctx, std::string &err) {
    if (pf_create(device, ctx) == PF_OK) return 0;
    err = std::string("trim: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); reads are trimmed on the GPU only";
    return 1;
}

// "who: [file f: ]record R of the chunk: clause" of the device call as the sub-command words it
std::string reword(pf_ctx *ctx, const std::string &who, const std::string &path, uint64_t record_1based) {
    const std::string why = pf_last_error(ctx);
    const size_t at = why.find("of the chunk: ");
    return at != std::string::npos ? who + ": " + path + ": record " + std::to_string(record_1based) + ": " + why.substr(at + 14) : who + ": " + path + ": " + why;
}

// ---- the pair loop's threads ----
struct ReadBlock {
    std::unique_ptr<char[]> p;
    uint64_t len = 0;
    bool eof = false;
    GzBlock g;   // of a blocked-gzip file: `len` bytes of whole members
};
struct PairReader {   // reads one file in blocks of `chunk` bytes, at most two ahead of the device stage
    Chan<int> tokens;
    Chan<ReadBlock> blocks;
    std::string err;
    double read_s = 0;
    std::thread th;
    void start(const std::string &who, const std::string &path, uint64_t chunk, bool gz) {
        tokens.push(0);
        tokens.push(0);
        if (gz) {   // whole members, hopped by BSIZE; nothing is decoded here
            th = std::thread([this, who, path, chunk] {
                GzReader gr;
                if (!gr.open_file(who, path, err)) { blocks.close(); return; }
                const uint64_t cap = gz_buffer_bytes(chunk);
                for (bool eof = false; !eof;) {
                    int token;
                    if (!tokens.pop(token)) break;
                    ReadBlock b;
                    b.p.reset(new char[cap]);
                    const auto t0 = clk::now();
                    const bool ok = gr.next(b.p.get(), cap, chunk, b.g, err);
                    read_s += since(t0);
                    if (!ok) break;
                    b.len = b.g.len;
                    eof = b.eof = b.g.eof;
                    blocks.push(std::move(b));
                }
                blocks.close();
            });
            return;
        }
        th = std::thread([this, who, path, chunk] {
            const int fd = open(path.c_str(), O_RDONLY);
            if (fd < 0) { err = who + ": cannot read " + path + " (" + strerror(errno) + ")"; blocks.close(); return; }
            for (bool eof = false; !eof;) {
                int token;
                if (!tokens.pop(token)) break;
                ReadBlock b;
                b.p.reset(new char[chunk]);
                const auto t0 = clk::now();
                while (b.len < chunk) {
                    const ssize_t got = read(fd, b.p.get() + b.len, (size_t)(chunk - b.len));
                    if (got < 0 && errno == EINTR) continue;
                    if (got < 0) { err = who + ": reading " + path + " (" + strerror(errno) + ")"; break; }
                    if (got == 0) { eof = true; break; }
                    b.len += (uint64_t)got;
                }
                read_s += since(t0);
                if (!err.empty()) break;
                b.eof = eof;
                blocks.push(std::move(b));
            }
            close(fd);
            blocks.close();
        });
    }
    void stop() {
        tokens.close();
        if (th.joinable()) th.join();
    }
};
struct WritePiece {
    std::shared_ptr<char> p;
    uint64_t len = 0;
};
struct PairWriter {   // writes the pieces of one output in order, at most two behind the device stage
    Chan<int> tokens;
    Chan<WritePiece> pieces;
    std::string err;
    double write_s = 0;
    std::thread th;
    void start(int fd, const std::string &name) {
        tokens.push(0);
        tokens.push(0);
        th = std::thread([this, fd, name] {
            WritePiece w;
            while (pieces.pop(w)) {
                const auto t0 = clk::now();
                if (err.empty()) write_all(fd, w.p.get(), w.len, name, err);
                write_s += since(t0);
                w.p.reset();
                tokens.push(0);
            }
        });
    }
    void put(WritePiece w) {
        int token;
        if (tokens.pop(token)) pieces.push(std::move(w));
    }
    void stop() {
        pieces.close();
        if (th.joinable()) th.join();
        tokens.close();
    }
};

}  // namespace

int trim_options_clause(const TrimOptions &opt, std::string &err) {
    uint32_t bad = 0;
    const int c = pf_trim::steps_clause(reinterpret_cast<const pf_trim::Step *>(opt.steps.data()), (uint32_t)opt.steps.size(), opt.phred, &bad);
    if (!c) return 0;
    err = std::string("trim: ") + pf_trim::refusal_text(c);
    if (c == pf_trim::REFUSE_PHRED) err += ", not " + std::to_string(opt.phred);
    else if (c != pf_trim::REFUSE_NO_STEP && c != pf_trim::REFUSE_TOO_MANY) err += " (step " + std::to_string(bad + 1) + ")";
    return c;
}

int trim_fastq(const std::vector<std::string> &inputs, const std::string &out_path, const TrimOptions &opt, int device, pf_trim_stats &stats,
               TrimTimes *times, std::string &err) {
    stats = pf_trim_stats{};
    err.clear();
    const bool logs = !opt.trimlog.empty();
    std::vector<std::string> paths = {out_path};
    if (logs) paths.push_back(opt.trimlog);
    uint64_t largest = 0;
    if (trim_preflight(inputs, paths, opt, largest, err)) return 1;
    pf_ctx *ctx = nullptr;
    if (trim_create(device, &ctx, err)) return 1;
    struct CtxGuard { pf_ctx *c; ~CtxGuard() { pf_destroy(c); } } ctx_guard{ctx};
    const auto t_stream = clk::now();
    OutFiles outs;
    if (outs.open_all(paths, err)) return 1;
    std::vector<uint32_t> rb, rl;
    std::vector<uint64_t> lb, le;
    std::string log, log_err;
    std::vector<char> fetched;
    StreamTimes st_tm;
    stream_fastq_sized(ctx, "trim", inputs, opt.chunk_bytes, largest, outs.f[0].fd, outs.f[0].tmp,
                       [&](const char *text, uint64_t n, bool final, char *out, uint64_t &used, uint64_t &reads, uint64_t &bad, uint64_t &out_len) {
                           if (logs) { rb.resize(n / 4 + 1); rl.resize(n / 4 + 1); }
                           pf_trim_stats st = {};
                           const int rc = pf_trim_fastq(ctx, text, n, final ? 1 : 0, opt.steps.data(), (uint32_t)opt.steps.size(), opt.phred, out, &out_len,
                                                        &used, logs ? rb.data() : nullptr, logs ? rl.data() : nullptr, &reads, &st, &bad);
                           if (rc != PF_OK) return rc;
                           add_stats(stats, st);
                           if (logs && log_err.empty()) {   // on the host, from the (begin, len) arrays
                               if (st_tm.text_on_device) {   // (inflated on the device: the log alone takes the text across)
                                   fetched.resize(used);
                                   if (used && pf_copy(ctx, fetched.data(), text, (size_t)used) != PF_OK) return (int)PF_ERR_HIP;
                                   text = fetched.data();
                               }
                               pf_trim::record_lines(text, used, reads, lb, le);
                               log.clear();
                               for (uint64_t r = 0; r < reads; ++r) trimlog_line(log, text, &lb[4 * r], &le[4 * r], rb[r], rl[r]);
                               write_all(outs.f[1].fd, log.data(), log.size(), outs.f[1].tmp, log_err);
                           }
                           return (int)PF_OK;
                       },
                       st_tm, err, opt.gz);
    if (err.empty()) err = log_err;
    if (!err.empty() || outs.commit(err)) return 1;
    if (times) {
        times->stream_s = since(t_stream);
        times->device_s = st_tm.device_s;
        times->read_s = st_tm.read_s;
        times->write_s = st_tm.write_s;
    }
    return 0;
}

int stream_fastq_pair(pf_ctx *ctx, const char *who_c, const std::string &in1, const std::string &in2, uint64_t chunk_bytes, uint64_t largest,
                      const PairChunkStep &step, PairStreamTimes &tm, std::string &err, int gz) {
    const std::string who = who_c;
    const std::string inputs[2] = {in1, in2};
    err.clear();
    const int kind[2] = {gz_kind(in1, gz), gz_kind(in2, gz)};   // (each file of the pair by its own first bytes)
    const bool is_gz[2] = {kind[0] != GZ_KIND_TEXT, kind[1] != GZ_KIND_TEXT};
    // a call holds what is pending of each file, up to two blocks of it: both stay below the 2^32 bytes of the device call
    uint64_t chunk = chunk_bytes ? chunk_bytes : MASK_DEFAULT_CHUNK;
    const uint64_t bound = (is_gz[0] || is_gz[1]) ? std::max<uint64_t>(largest * 8, GZ_MEMBER_MAX) : largest;   // (blocked gzip inflates to a multiple of the file)
    chunk = std::max<uint64_t>(1, std::min<uint64_t>(chunk, std::max<uint64_t>(bound, 1)));
    chunk = std::min<uint64_t>(chunk, 1ull << 30);
    PairReader rd[2];
    // (a plain-gzip file is read as it is, in smaller blocks: its text is several times its bytes)
    rd[0].start(who, in1, kind[0] == GZ_KIND_GZIP ? gz_plain_block(chunk) : chunk, kind[0] == GZ_KIND_BGZF);
    rd[1].start(who, in2, kind[1] == GZ_KIND_GZIP ? gz_plain_block(chunk) : chunk, kind[1] == GZ_KIND_BGZF);
    uint64_t raw_off[2] = {0, 0};   // bytes of a plain-gzip file handed over so far

    std::vector<char> pend[2];             // the carry of each file, then the blocks read behind it
    std::unique_ptr<GzText> gzt[2];        // the same of a blocked-gzip file: on the device
    for (int f = 0; f < 2; ++f)
        if (is_gz[f]) gzt[f].reset(new GzText(ctx));
    auto size_of = [&](int f) { return is_gz[f] ? gzt[f]->size() : (uint64_t)pend[f].size(); };
    auto text_of = [&](int f) { return is_gz[f] ? gzt[f]->text() : pend[f].data(); };
    bool eof[2] = {false, false}, more[2] = {true, true};
    uint64_t records_before = 0;           // pairs in front of the current call
    // whole records of what is pending of file f (on the host: only when the other file has ended)
    auto whole_records = [&](int f) {
        uint64_t used = 0, recs = 0, bad = 0;
        std::vector<char> fetched;
        std::string e;
        if (is_gz[f]) (void)gzt[f]->fetch(fetched, e);
        const std::vector<char> &t = is_gz[f] ? fetched : pend[f];
        (void)pf_mask::index_fastq(t.data(), t.size(), eof[f], used, recs, bad);
        return recs;
    };
    while (err.empty()) {
        // ---- each file grows by a block while it holds less than a chunk, or held no whole record the last time ----
        for (int f = 0; f < 2 && err.empty(); ++f)
            while (!eof[f] && (size_of(f) < chunk || more[f])) {
                ReadBlock b;
                if (!rd[f].blocks.pop(b)) { err = !rd[f].err.empty() ? rd[f].err : who + ": reading " + inputs[f] + " ended early"; break; }
                if (is_gz[f]) {
                    const auto t0 = clk::now();
                    const bool ok = kind[f] == GZ_KIND_GZIP ? gzt[f]->append_plain(who, inputs[f], b.p.get(), b.len, raw_off[f], b.eof, err)
                                                            : gzt[f]->append(who, inputs[f], b.p.get(), b.g, err);
                    raw_off[f] += b.len;
                    tm.device_s += since(t0);
                    if (!ok) break;
                } else {
                    pend[f].insert(pend[f].end(), b.p.get(), b.p.get() + b.len);
                }
                eof[f] = b.eof;
                more[f] = false;
                b.p.reset();
                rd[f].tokens.push(0);
            }
        if (!err.empty()) break;
        const bool final = eof[0] && eof[1];
        if (final && size_of(0) == 0 && size_of(1) == 0) break;
        // ---- one file has ended and is used up while the other still holds a whole record ----
        for (int f = 0; f < 2 && !final; ++f)
            if (eof[f] && size_of(f) == 0 && whole_records(1 - f)) {
                err = who + ": " + inputs[f] + " ends after " + std::to_string(records_before) + " records while " + inputs[1 - f] + " holds more (at least " +
                      std::to_string(records_before + whole_records(1 - f)) + "): the files of a pair hold the same number of records";
            }
        if (!err.empty()) break;
        // ---- the device stage ----
        uint64_t used[2] = {0, 0}, recs = 0, bad = 0;
        tm.text_on_device[0] = is_gz[0];
        tm.text_on_device[1] = is_gz[1];
        const auto t0 = clk::now();
        const int rc = step(text_of(0), size_of(0), text_of(1), size_of(1), final, used, recs, bad);
        tm.device_s += since(t0);
        if (rc != PF_OK) {
            if (!err.empty()) break;   // (the step has worded it)
            const std::string why = pf_last_error(ctx);
            if (why.find("different numbers of records") != std::string::npos)
                err = who + ": " + in1 + " holds " + std::to_string(records_before + whole_records(0)) + " records, " + in2 + " holds " +
                      std::to_string(records_before + whole_records(1)) + ": the files of a pair hold the same number of records";
            else
                err = reword(ctx, who, inputs[bad & 1], records_before + (bad >> 1) + 1);
            break;
        }
        for (int f = 0; f < 2; ++f) {
            if (is_gz[f]) gzt[f]->use(used[f]);
            else pend[f].erase(pend[f].begin(), pend[f].begin() + (ptrdiff_t)used[f]);
        }
        records_before += recs;
        if (final) break;
        if (recs == 0) more[0] = more[1] = true;   // no whole pair: a file that can grows by the next block
    }
    // wind down: on an error the threads are let go first
    for (int f = 0; f < 2; ++f) rd[f].stop();
    for (int f = 0; f < 2 && err.empty(); ++f) err = rd[f].err;
    tm.read_s = std::max(rd[0].read_s, rd[1].read_s);
    return err.empty() ? 0 : 1;
}

int trim_fastq_pair(const std::string &in1, const std::string &in2, const std::string out_paths[4], const TrimOptions &opt, int device,
                    pf_trim_stats stats[2], TrimTimes *times, std::string &err) {
    stats[0] = stats[1] = pf_trim_stats{};
    err.clear();
    const bool logs = !opt.trimlog.empty();
    const std::vector<std::string> inputs = {in1, in2};
    std::vector<std::string> paths(out_paths, out_paths + 4);
    if (logs) paths.push_back(opt.trimlog);
    uint64_t largest = 0;
    if (trim_preflight(inputs, paths, opt, largest, err)) return 1;
    if (same_file(in1, in2)) { err = "trim: the two inputs of a pair are the same file (" + in1 + ")"; return 1; }
    pf_ctx *ctx = nullptr;
    if (trim_create(device, &ctx, err)) return 1;
    struct CtxGuard { pf_ctx *c; ~CtxGuard() { pf_destroy(c); } } ctx_guard{ctx};
    const auto t_stream = clk::now();
    OutFiles outs;
    if (outs.open_all(paths, err)) return 1;

    PairWriter wr[4];
    for (int d = 0; d < 4; ++d) wr[d].start(outs.f[d].fd, outs.f[d].tmp);
    std::vector<uint32_t> rb[2], rl[2];
    std::vector<uint64_t> lb[2], le[2];
    std::string log;
    std::vector<char> fetched[2];
    PairStreamTimes ptm;
    stream_fastq_pair(ctx, "trim", in1, in2, opt.chunk_bytes, largest,
                      [&](const char *t1, uint64_t n1, const char *t2, uint64_t n2, bool final, uint64_t used[2], uint64_t &recs, uint64_t &bad) {
                          const char *text[2] = {t1, t2};
                          const uint64_t n[2] = {n1, n2};
                          std::shared_ptr<char> out[4];
                          char *out_p[4];
                          for (int d = 0; d < 4; ++d) {
                              out[d] = std::shared_ptr<char>(new char[n[d / 2] + 1], std::default_delete<char[]>());
                              out_p[d] = out[d].get();
                          }
                          uint32_t *rb_p[2] = {nullptr, nullptr}, *rl_p[2] = {nullptr, nullptr};
                          if (logs)
                              for (int f = 0; f < 2; ++f) {
                                  rb[f].resize(n[f] / 4 + 1);
                                  rl[f].resize(n[f] / 4 + 1);
                                  rb_p[f] = rb[f].data();
                                  rl_p[f] = rl[f].data();
                              }
                          uint64_t out_bytes[4] = {0, 0, 0, 0};
                          pf_trim_stats st[2] = {};
                          const int rc = pf_trim_fastq_pair(ctx, t1, n1, t2, n2, final ? 1 : 0, opt.steps.data(), (uint32_t)opt.steps.size(), opt.phred, out_p,
                                                            out_bytes, used, rb_p, rl_p, &recs, st, &bad);
                          if (rc != PF_OK) return rc;
                          add_stats(stats[0], st[0]);
                          add_stats(stats[1], st[1]);
                          if (logs) {
                              log.clear();
                              for (int f = 0; f < 2; ++f)
                                  if (ptm.text_on_device[f]) {   // (inflated on the device: the log alone takes the text across)
                                      fetched[f].resize(used[f]);
                                      if (used[f] && pf_copy(ctx, fetched[f].data(), text[f], (size_t)used[f]) != PF_OK) return (int)PF_ERR_HIP;
                                      text[f] = fetched[f].data();
                                  }
                              for (int f = 0; f < 2; ++f) pf_trim::record_lines(text[f], used[f], recs, lb[f], le[f]);
                              for (uint64_t r = 0; r < recs; ++r)
                                  for (int f = 0; f < 2; ++f) trimlog_line(log, text[f], &lb[f][4 * r], &le[f][4 * r], rb[f][r], rl[f][r]);
                              if (!write_all(outs.f[4].fd, log.data(), log.size(), outs.f[4].tmp, err)) return (int)PF_ERR_ARG;   // (err is worded)
                          }
                          for (int d = 0; d < 4; ++d)
                              if (out_bytes[d]) wr[d].put(WritePiece{out[d], out_bytes[d]});
                          return (int)PF_OK;
                      },
                      ptm, err, opt.gz);
    for (int d = 0; d < 4; ++d) wr[d].stop();
    for (int d = 0; d < 4 && err.empty(); ++d) err = wr[d].err;
    if (!err.empty() || outs.commit(err)) return 1;
    if (times) {
        times->stream_s = since(t_stream);
        times->device_s = ptm.device_s;
        times->read_s = ptm.read_s;
        times->write_s = wr[0].write_s + wr[1].write_s + wr[2].write_s + wr[3].write_s;
    }
    return 0;
}

}  // namespace pfh
