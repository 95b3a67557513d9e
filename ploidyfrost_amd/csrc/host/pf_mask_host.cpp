#include "pf_mask_host.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>

#include "../pf_mask_rule.hpp"
#include "pf_count_host.hpp"
#include "pf_cutoffs.hpp"
#include "pf_gz_host.hpp"
#include "../pf_inflate_rule.hpp"
#include "../pf_gunzip_rule.hpp"
#include "../pf_fasta_rule.hpp"
#include "pf_host_graph.hpp"

namespace pfh {

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

struct Block {     // reader -> device: bytes [HEAD, HEAD + len) of input buffer `buf`
    int buf = -1;
    uint64_t len = 0;
    size_t input = 0;
    bool eof = false;
    bool gz = false;   // blocked gzip: `len` bytes of whole members, described by g
    GzBlock g;
};
struct Piece {     // device -> writer: `len` bytes at `p`; buf >= 0: an output buffer to hand back, else `own` keeps them alive
    int buf = -1;
    const char *p = nullptr;
    uint64_t len = 0;
    std::shared_ptr<std::vector<char>> own;
};

constexpr uint64_t MASK_HEAD = 1u << 16;   // room in front of a block for the record carried over from the last one

}  // namespace

bool ChunkBuf::alloc(pf_ctx *c, size_t bytes) {
    ctx = c;
    void *v = nullptr;
    if (pf_host_alloc(c, bytes, &v) == PF_OK && v) { p = static_cast<char *>(v); pinned = true; return true; }
    p = static_cast<char *>(malloc(bytes));   // pageable memory works, slower
    return p != nullptr;
}
ChunkBuf::~ChunkBuf() {
    if (p && pinned) pf_host_free(ctx, p);
    else free(p);
}

bool same_file(const std::string &a, const std::string &b) {
    if (a == b) return true;
    struct stat sa, sb;
    return stat(a.c_str(), &sa) == 0 && stat(b.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}

int fastq_preflight(const char *who, const char *what, const std::vector<std::string> &inputs, const std::vector<std::string> &outputs,
                    uint64_t &largest, std::string &err, int gz, bool fasta) {
    const std::string w = who;
    auto text = [&](int clause) {   // (the FASTA and gzip texts end in what is done with FASTQ: "masked")
        std::string t = pf_mask::clause_text(clause);
        if (clause != pf_mask::CLAUSE_SAME_PATH && strcmp(what, "masked") != 0) t.replace(t.size() - 6, 6, what);
        return t;
    };
    largest = 0;
    if (inputs.empty()) { err = w + ": no input"; return 1; }
    std::vector<unsigned char> head(gz ? 65536 : 2);
    for (const std::string &in : inputs) {
        for (const std::string &out : outputs)
            if (same_file(in, out)) { err = w + ": " + in + ": " + text(pf_mask::CLAUSE_SAME_PATH); return 1; }
        const int fd = open(in.c_str(), O_RDONLY);
        if (fd < 0) { err = w + ": cannot read " + in + " (" + strerror(errno) + ")"; return 1; }
        unsigned char *first = head.data();
        ssize_t got = read(fd, first, 2);
        struct stat st;
        uint64_t size = 0;
        if (fstat(fd, &st) == 0) size = (uint64_t)st.st_size;
        largest = std::max<uint64_t>(largest, size);
        if (gz && got == 2 && first[0] == 0x1f && first[1] == 0x8b) {   // with --gz: blocked gzip, or refused by name
            while ((size_t)got < head.size()) {
                const ssize_t more = read(fd, first + got, head.size() - (size_t)got);
                if (more < 0 && errno == EINTR) continue;
                if (more <= 0) break;
                got += more;
            }
            close(fd);
            int clause = 0;
            if (gz == 2) {   // --gz-plain: blocked gzip as with --gz, any other gzip by its own header
                if (pf_gunzip::file_kind(first, (uint64_t)got, std::max<uint64_t>(size, (uint64_t)got), &clause) == pf_gunzip::FILE_REFUSED) {
                    err = w + ": " + in + ": member 1, byte 0: " + pf_gunzip::clause_text(clause);
                    return 1;
                }
                continue;
            }
            if (pf_inflate::file_clause_gz(first, (uint64_t)got, std::max<uint64_t>(size, (uint64_t)got), &clause) == pf_inflate::FILE_REFUSED) {
                err = w + ": " + in + ": member 1, byte 0: " + pf_inflate::clause_text(clause);
                return 1;
            }
            continue;
        }
        close(fd);
        const int clause = pf_mask::file_clause(first, got > 0 ? (uint64_t)got : 0);
        if (clause && !(fasta && clause == pf_mask::CLAUSE_FASTA)) { err = w + ": " + in + ": record 1: " + text(clause); return 1; }
    }
    return 0;
}

bool chunk_is_fasta(pf_ctx *ctx, const char *text, uint64_t n, bool on_device) {
    if (!n) return false;
    char first = 0;
    if (!on_device) first = text[0];
    else if (pf_copy_to_host(ctx, &first, text, 1) != PF_OK) return false;   // (the FASTQ call reports what is wrong with the context)
    return first == pf_fasta::HEADER_BYTE;
}

int stream_fastq(pf_ctx *ctx, const char *who, const std::vector<std::string> &inputs, uint64_t chunk_bytes, uint64_t largest, int out_fd,
                 const std::string &out_name, const ChunkStep &step, StreamTimes &tm, std::string &err, int gz) {
    return stream_fastq_sized(ctx, who, inputs, chunk_bytes, largest, out_fd, out_name,
                              [&](const char *text, uint64_t n, bool final, char *out, uint64_t &used, uint64_t &reads, uint64_t &bad, uint64_t &out_len) {
                                  const int rc = step(text, n, final, out, used, reads, bad);
                                  out_len = used;
                                  return rc;
                              },
                              tm, err, gz);
}

int stream_fastq_sized(pf_ctx *ctx, const char *who_c, const std::vector<std::string> &inputs, uint64_t chunk_bytes, uint64_t largest, int out_fd,
                       const std::string &out_name, const SizedChunkStep &step, StreamTimes &tm, std::string &err, int gz) {
    const std::string who = who_c;
    err.clear();   // (a caller's `err` may still hold the text of an earlier call: the loop below runs while it is empty)
    const bool writes = out_fd >= 0;
    uint64_t chunk = chunk_bytes ? chunk_bytes : MASK_DEFAULT_CHUNK;
    std::vector<char> is_gz(inputs.size(), 0);   // with --gz: the inputs that start with the gzip magic are blocked gzip (the preflight has looked)
    bool any_gz = false;
    for (size_t f = 0; gz && f < inputs.size(); ++f) any_gz |= (is_gz[f] = (char)gz_kind(inputs[f], gz)) != 0;   // (--gz-plain: GZ_KIND_GZIP beside them)
    // (no gigabyte of pinned memory for a small file; a blocked-gzip file inflates to a multiple of its size)
    chunk = std::max<uint64_t>(1, std::min<uint64_t>(chunk, std::max<uint64_t>(any_gz ? std::max<uint64_t>(largest * 8, GZ_MEMBER_MAX) : largest, 1)));
    chunk = std::min<uint64_t>(chunk, 1ull << 31);                                               // a chunk and its carry stay below the 2^32 of the device calls
    const uint64_t in_bytes = any_gz ? std::max(chunk, gz_buffer_bytes(chunk)) : chunk;          // (--chunk-bytes counts inflated bytes)
    ChunkBuf in_buf[2], out_buf[2];
    for (int i = 0; i < 2; ++i)
        if (!in_buf[i].alloc(ctx, MASK_HEAD + in_bytes) || (writes && !out_buf[i].alloc(ctx, MASK_HEAD + chunk + 16))) { err = who + ": no memory for the chunk buffers"; return 1; }

    Chan<int> free_in, free_out;
    Chan<Block> blocks;
    Chan<Piece> pieces;
    for (int i = 0; i < 2; ++i) { free_in.push(i); free_out.push(i); }
    std::string read_err, write_err;
    double read_s = 0, write_s = 0;
    // reader: the next block of the next input is read while the device works on this one
    std::thread reader([&] {
        for (size_t f = 0; f < inputs.size(); ++f) {
            if (is_gz[f]) {   // whole members, hopped by BSIZE; nothing is decoded here
                GzReader gr;
                if (!gr.open_file(who, inputs[f], read_err)) break;
                for (bool eof = false; !eof;) {
                    Block b;
                    if (!free_in.pop(b.buf)) return;
                    b.input = f;
                    b.gz = true;
                    const auto t0 = clk::now();
                    const bool ok = is_gz[f] == GZ_KIND_GZIP ? gr.next_raw(in_buf[b.buf].p + MASK_HEAD, std::min(in_bytes, gz_plain_block(chunk)), b.g, read_err)
                                                             : gr.next(in_buf[b.buf].p + MASK_HEAD, in_bytes, chunk, b.g, read_err);
                    read_s += since(t0);
                    if (!ok) { blocks.close(); return; }
                    b.len = b.g.len;
                    eof = b.eof = b.g.eof;
                    blocks.push(std::move(b));
                }
                continue;
            }
            const int fd = open(inputs[f].c_str(), O_RDONLY);
            if (fd < 0) { read_err = who + ": cannot read " + inputs[f] + " (" + strerror(errno) + ")"; break; }
            for (bool eof = false; !eof;) {
                Block b;
                if (!free_in.pop(b.buf)) { close(fd); return; }
                b.input = f;
                const auto t0 = clk::now();
                while (b.len < chunk) {
                    const ssize_t got = read(fd, in_buf[b.buf].p + MASK_HEAD + b.len, (size_t)(chunk - b.len));
                    if (got < 0 && errno == EINTR) continue;
                    if (got < 0) { read_err = who + ": reading " + inputs[f] + " (" + strerror(errno) + ")"; break; }
                    if (got == 0) { eof = true; break; }
                    b.len += (uint64_t)got;
                }
                read_s += since(t0);
                if (!read_err.empty()) { close(fd); blocks.close(); return; }
                b.eof = eof;
                blocks.push(b);
            }
            close(fd);
        }
        blocks.close();
    });
    // writer (only with an output): the last piece is written while the device works on this one
    std::thread writer;
    if (writes) writer = std::thread([&] {
        Piece p;
        while (pieces.pop(p)) {
            const auto t0 = clk::now();
            for (uint64_t done = 0; done < p.len && write_err.empty();) {
                const ssize_t put = write(out_fd, p.p + done, (size_t)(p.len - done));
                if (put < 0 && errno == EINTR) continue;
                if (put < 0) { write_err = who + ": writing " + out_name + " (" + strerror(errno) + ")"; break; }
                done += (uint64_t)put;
            }
            write_s += since(t0);
            if (p.buf >= 0) free_out.push(p.buf);
        }
    });

    // device: carry + block -> step -> piece
    std::vector<char> carry;
    std::unique_ptr<GzText> gzt;   // blocked gzip: the text and its carry stay on the device
    uint64_t records_before = 0;   // whole records of the current input in front of the current chunk
    size_t cur_input = 0;
    Block b;
    while (err.empty() && blocks.pop(b)) {
        if (b.input != cur_input) { cur_input = b.input; records_before = 0; }
        uint64_t n = carry.size() + b.len;
        const char *text;
        char *out = nullptr;
        Piece piece;
        std::shared_ptr<std::vector<char>> big_in;
        if (b.gz) {
            if (!gzt) gzt.reset(new GzText(ctx));
            const auto t0 = clk::now();
            const bool ok = b.g.plain ? gzt->append_plain(who, inputs[b.input], in_buf[b.buf].p + MASK_HEAD, b.g.len, b.g.file_off, b.g.eof, err)
                                      : gzt->append(who, inputs[b.input], in_buf[b.buf].p + MASK_HEAD, b.g, err);
            tm.device_s += since(t0);
            if (!ok) break;
            text = gzt->text();
            n = gzt->size();
            if (writes && n + 1 <= MASK_HEAD + chunk + 16) {
                if (!free_out.pop(piece.buf)) break;
                out = out_buf[piece.buf].p;
            } else if (writes) {
                piece.own = std::make_shared<std::vector<char>>(n + 1);
                out = piece.own->data();
            }
        } else if (carry.size() <= MASK_HEAD) {   // the carried record in front of the block, in place
            char *p = in_buf[b.buf].p + MASK_HEAD - carry.size();
            memcpy(p, carry.data(), carry.size());
            text = p;
            if (writes) {
                if (!free_out.pop(piece.buf)) break;
                out = out_buf[piece.buf].p;
            }
        } else {   // a record longer than the room in front: this chunk holds what has gathered so far
            big_in = std::make_shared<std::vector<char>>(n);
            memcpy(big_in->data(), carry.data(), carry.size());
            memcpy(big_in->data() + carry.size(), in_buf[b.buf].p + MASK_HEAD, b.len);
            text = big_in->data();
            if (writes) {
                piece.own = std::make_shared<std::vector<char>>(n + 1);
                out = piece.own->data();
            }
        }
        tm.text_on_device = b.gz;
        uint64_t used = 0, bad = 0, reads = 0, out_len = 0;
        const auto t0 = clk::now();
        const int rc = n ? step(text, n, b.eof, out, used, reads, bad, out_len) : (int)PF_OK;
        tm.device_s += since(t0);
        if (rc != PF_OK) {
            const std::string why = pf_last_error(ctx);
            const size_t at = why.find("of the chunk: ");
            err = at != std::string::npos
                      ? who + ": " + inputs[b.input] + ": record " + std::to_string(records_before + bad + 1) + ": " + why.substr(at + 14)
                      : who + ": " + inputs[b.input] + ": " + why;
            if (piece.buf >= 0) free_out.push(piece.buf);
            break;
        }
        // a chunk that holds no whole record gives used = 0: everything is carried and the next chunk is this one plus the next block
        if (b.gz) gzt->use(used);
        else carry.assign(text + used, text + n);
        free_in.push(b.buf);
        records_before += reads;
        piece.p = out;
        piece.len = out_len;
        if (writes) pieces.push(std::move(piece));
    }
    // wind down: on an error the threads are let go first
    free_in.close();
    blocks.close();
    reader.join();
    pieces.close();
    if (writes) writer.join();
    free_out.close();
    if (err.empty()) err = !read_err.empty() ? read_err : write_err;
    tm.read_s = read_s;
    tm.write_s = write_s;
    return err.empty() ? 0 : 1;
}

namespace {

// the table is resident: the inputs through K-MASK into out_path
int mask_stream(pf_ctx *ctx, const std::vector<std::string> &inputs, const std::string &out_path, uint32_t low, uint32_t up, uint64_t chunk_bytes,
                uint64_t largest, pf_mask_stats &stats, MaskTimes &tm, std::string &err) {
    const auto t_stream = clk::now();
    const std::string tmp_path = out_path + ".tmp." + std::to_string((long)getpid());
    const int out_fd = open(tmp_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (out_fd < 0) { err = "mask: cannot write " + tmp_path + " (" + strerror(errno) + ")"; return 1; }
    StreamTimes st_tm;
    stream_fastq(ctx, "mask", inputs, chunk_bytes, largest, out_fd, tmp_path,
                 [&](const char *text, uint64_t n, bool final, char *out, uint64_t &used, uint64_t &reads, uint64_t &bad) {
                     pf_mask_stats st = {};
                     const int rc = pf_mask_fastq(ctx, text, n, final ? 1 : 0, low, up, out, &used, &st, &bad);
                     if (rc != PF_OK) return rc;
                     reads = st.reads;
                     stats.reads += st.reads;
                     stats.reads_changed += st.reads_changed;
                     stats.bases += st.bases;
                     stats.bases_masked += st.bases_masked;
                     stats.kmers += st.kmers;
                     stats.kmers_bad += st.kmers_bad;
                     return (int)PF_OK;
                 },
                 st_tm, err);
    if (err.empty() && close(out_fd) != 0) err = "mask: closing " + tmp_path + " (" + strerror(errno) + ")";
    else if (!err.empty()) close(out_fd);
    if (err.empty() && rename(tmp_path.c_str(), out_path.c_str()) != 0) err = "mask: renaming " + tmp_path + " to " + out_path + " (" + strerror(errno) + ")";
    if (!err.empty()) { unlink(tmp_path.c_str()); return 1; }
    tm.stream_s = since(t_stream);
    tm.device_s = st_tm.device_s;
    tm.read_s = st_tm.read_s;
    tm.write_s = st_tm.write_s;
    return 0;
}

// the thresholds once the rows of the histogram are known
int mask_auto_lower(const std::vector<uint64_t> &rows, uint32_t &low, uint32_t up, uint32_t &lower_used, std::string &err) {
    int lo = 0, hi = 0;
    (void)cutoffs_from_rows(rows, 0.998, lo, hi);
    lower_used = low = (uint32_t)std::max(10, lo);
    if (low > up) { err = "mask: the derived lower threshold " + std::to_string(low) + " is above the upper threshold " + std::to_string(up); return 1; }
    return 0;
}

int mask_create(int device, pf_ctx **ctx, std::string &err) {
    if (pf_create(device, ctx) == PF_OK) return 0;
    err = std::string("mask: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); reads are masked on the GPU only";
    return 1;
}

}  // namespace

int mask_fastq(const std::string &db_prefix, const std::vector<std::string> &inputs, const std::string &out_path, uint32_t low, uint32_t up,
               bool auto_lower, uint64_t chunk_bytes, int device, pf_mask_stats &stats, uint32_t &lower_used, MaskTimes *times, std::string &err) {
    stats = pf_mask_stats{};
    lower_used = low;
    MaskTimes tm;
    // ---- refusals that need no device: every input is looked at before anything is written ----
    if (inputs.empty()) { err = "mask: no input"; return 1; }
    if (out_path.empty()) { err = "mask: no output path"; return 1; }
    uint64_t largest = 0;
    if (fastq_preflight("mask", "masked", inputs, {out_path}, largest, err)) return 1;
    if (!auto_lower && low > up) { err = "mask: the lower threshold " + std::to_string(low) + " is above the upper threshold " + std::to_string(up); return 1; }

    // ---- load: the database once -- decode (K-KMC), with auto_lower its histogram (K-HIST), the table ----
    const auto t_load = clk::now();
    pf_ctx *ctx = nullptr;
    if (mask_create(device, &ctx, err)) return 1;
    struct CtxGuard { pf_ctx *c; ~CtxGuard() { pf_destroy(c); } } ctx_guard{ctx};
    {
        KmcRecords db;
        std::string e;
        if (!db.load(db_prefix, e)) { err = "Open kmc database " + db_prefix + " error (" + e + ")"; return 1; }
        uint64_t *dk = nullptr;
        uint32_t *dc = nullptr;
        int st = pf_kmc_decode(ctx, db.records, db.total, db.suffix_bytes, db.counter_size, db.lut.data(), db.n_lut(), db.lut_prefix_len, db.k, &dk, &dc);
        std::vector<uint64_t> rows;
        if (st == PF_OK && auto_lower) st = kmc_rows_of_counts(ctx, db, dc, rows);
        if (st == PF_OK) st = pf_upload_counts(ctx, dk, dc, db.total, db.k, db.min_count, db.max_count, db.both_strands);
        pf_device_free(ctx, dk);
        pf_device_free(ctx, dc);
        if (st != PF_OK) { err = "mask: count table of " + db_prefix + ": " + pf_last_error(ctx); return 1; }
        if (auto_lower && mask_auto_lower(rows, low, up, lower_used, err)) return 1;
    }
    tm.load_s = since(t_load);
    if (mask_stream(ctx, inputs, out_path, low, up, chunk_bytes, largest, stats, tm, err)) return 1;
    if (times) *times = tm;
    return 0;
}

int mask_fastq_counted(const CountOptions &count, const std::string &db_out, const std::vector<std::string> &inputs, const std::string &out_path,
                       uint32_t low, uint32_t up, bool auto_lower, uint64_t chunk_bytes, int device, pf_mask_stats &stats, uint32_t &lower_used,
                       MaskTimes *times, std::string &err) {
    stats = pf_mask_stats{};
    lower_used = low;
    MaskTimes tm;
    if (inputs.empty()) { err = "mask: no input"; return 1; }
    if (out_path.empty()) { err = "mask: no output path"; return 1; }
    std::vector<std::string> outputs = {out_path};
    if (!db_out.empty()) { outputs.push_back(db_out + ".kmc_pre"); outputs.push_back(db_out + ".kmc_suf"); }
    uint64_t largest = 0;
    if (fastq_preflight("mask", "masked", inputs, outputs, largest, err)) return 1;
    if (!auto_lower && low > up) { err = "mask: the lower threshold " + std::to_string(low) + " is above the upper threshold " + std::to_string(up); return 1; }
    { const int c = count_options_clause(count, !db_out.empty()); if (c) { err = std::string("mask: ") + pf_count::cut_text(c); return 1; } }

    // ---- load: the inputs counted (K-COUNT), with auto_lower the histogram of the finished counters (K-HIST), the table ----
    const auto t_load = clk::now();
    pf_ctx *ctx = nullptr;
    if (mask_create(device, &ctx, err)) return 1;
    struct CtxGuard { pf_ctx *c; ~CtxGuard() { pf_destroy(c); } } ctx_guard{ctx};
    {
        CountOptions opt = count;
        opt.chunk_bytes = chunk_bytes;
        Counted db;
        pf_count_stats cst = {};
        CountTimes ctm;
        if (count_stream(ctx, "mask", inputs, opt, largest, db, cst, ctm, err)) return 1;
        struct Free { pf_ctx *c; Counted &d; ~Free() { pf_device_free(c, d.kmers); pf_device_free(c, d.counts); } } free_db{ctx, db};
        std::vector<uint64_t> rows;
        int st = auto_lower ? counted_rows(ctx, db, opt, rows) : (int)PF_OK;
        if (st == PF_OK) st = pf_upload_counts(ctx, db.kmers, db.counts, db.n, opt.k, opt.ci, opt.cx, opt.both_strands ? 1 : 0);
        if (st != PF_OK) { err = std::string("mask: count table of the inputs: ") + pf_last_error(ctx); return 1; }
        if (auto_lower && mask_auto_lower(rows, low, up, lower_used, err)) return 1;
        if (!db_out.empty() && write_counted(ctx, "mask", db_out, db, opt, err)) return 1;
    }
    tm.load_s = since(t_load);
    if (mask_stream(ctx, inputs, out_path, low, up, chunk_bytes, largest, stats, tm, err)) {
        if (!db_out.empty()) { unlink((db_out + ".kmc_pre").c_str()); unlink((db_out + ".kmc_suf").c_str()); }   // nothing is left after a refusal
        return 1;
    }
    if (times) *times = tm;
    return 0;
}

}  // namespace pfh
