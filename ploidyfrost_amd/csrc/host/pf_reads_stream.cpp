#include "pf_reads_stream.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <memory>
#include <thread>

#include "../pf_fasta_rule.hpp"
#include "../pf_gunzip_rule.hpp"
#include "../pf_inflate_rule.hpp"
#include "../pf_mask_rule.hpp"
#include "pf_host_util.hpp"

namespace pfh {

namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

struct Block {     // reader -> device: bytes [HEAD, HEAD + g.len) of input buffer `buf`
    int buf = -1;
    size_t input = 0;
    FileBlock g;
};
struct Piece {     // device -> writer: `len` bytes at `p`; buf >= 0: an output buffer to hand back, else `own` keeps them alive
    int buf = -1;
    const char *p = nullptr;
    uint64_t len = 0;
    std::shared_ptr<std::vector<char>> own;
};

constexpr uint64_t MASK_HEAD = 1u << 16;   // room in front of a block for the record carried over from the last one

// `--fasta`: the kind of a chunk is its first byte
bool starts_fasta(pf_ctx *ctx, const char *text, uint64_t n, bool on_device) {
    if (!n) return false;
    char first = 0;
    if (!on_device) first = text[0];
    else if (pf_copy_to_host(ctx, &first, text, 1) != PF_OK) return false;   // (the FASTQ call reports what is wrong with the context)
    return first == pf_fasta::HEADER_BYTE;
}

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

int fastq_preflight(const char *who, const char *what, const std::vector<std::string> &paths, const std::vector<std::string> &outputs,
                    const ReadsOptions &opt, std::vector<ReadsInput> &inputs, std::string &err) {
    const std::string w = who;
    auto text = [&](int clause) {   // (the FASTA and gzip texts end in what is done with FASTQ: "masked")
        std::string t = pf_mask::clause_text(clause);
        if (clause != pf_mask::CLAUSE_SAME_PATH && strcmp(what, "masked") != 0) t.replace(t.size() - 6, 6, what);
        return t;
    };
    inputs.clear();
    if (paths.empty()) { err = w + ": no input"; return 1; }
    std::vector<unsigned char> head(opt.gz ? 65536 : 2);
    for (const std::string &path : paths) {
        for (const std::string &out : outputs)
            if (same_file(path, out)) { err = w + ": " + path + ": " + text(pf_mask::CLAUSE_SAME_PATH); return 1; }
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) { err = w + ": cannot read " + path + " (" + strerror(errno) + ")"; return 1; }
        ReadsInput in;
        in.path = path;
        in.fasta = opt.fasta;
        unsigned char *first = head.data();
        ssize_t got = read(fd, first, 2);
        struct stat st;
        if (fstat(fd, &st) == 0) in.size = (uint64_t)st.st_size;
        if (opt.gz && got == 2 && first[0] == 0x1f && first[1] == 0x8b) {   // with --gz: blocked gzip, or refused by name
            while ((size_t)got < head.size()) {
                const ssize_t more = read(fd, first + got, head.size() - (size_t)got);
                if (more < 0 && errno == EINTR) continue;
                if (more <= 0) break;
                got += more;
            }
            close(fd);
            const uint64_t size = std::max<uint64_t>(in.size, (uint64_t)got);
            int clause = 0;
            in.kind = GZ_KIND_BGZF;
            if (opt.gz == 2) {   // --gz-plain: blocked gzip as with --gz, any other gzip by its own header
                const int kind = pf_gunzip::file_kind(first, (uint64_t)got, size, &clause);
                if (kind == pf_gunzip::FILE_REFUSED) { err = w + ": " + path + ": member 1, byte 0: " + pf_gunzip::clause_text(clause); return 1; }
                if (kind == pf_gunzip::FILE_GZIP) in.kind = GZ_KIND_GZIP;
            } else if (pf_inflate::file_clause_gz(first, (uint64_t)got, size, &clause) == pf_inflate::FILE_REFUSED) {
                err = w + ": " + path + ": member 1, byte 0: " + pf_inflate::clause_text(clause);
                return 1;
            }
            inputs.push_back(std::move(in));
            continue;
        }
        close(fd);
        const int clause = pf_mask::file_clause(first, got > 0 ? (uint64_t)got : 0);
        if (clause && !(opt.fasta && clause == pf_mask::CLAUSE_FASTA)) { err = w + ": " + path + ": record 1: " + text(clause); return 1; }
        inputs.push_back(std::move(in));
    }
    return 0;
}

int stream_fastq(pf_ctx *ctx, const char *who_c, const std::vector<ReadsInput> &inputs, uint64_t chunk_bytes, int out_fd, const std::string &out_name,
                 const ChunkStep &step, StreamTimes &tm, std::string &err) {
    const std::string who = who_c;
    err.clear();   // (a caller's `err` may still hold the text of an earlier call: the loop below runs while it is empty)
    const bool writes = out_fd >= 0;
    uint64_t chunk = chunk_bytes ? chunk_bytes : MASK_DEFAULT_CHUNK;
    bool any_gz = false;
    uint64_t largest = 0;
    for (const ReadsInput &in : inputs) {
        any_gz |= in.kind != GZ_KIND_TEXT;
        largest = std::max(largest, in.size);
    }
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
            BlockReader rd;
            if (!rd.open_file(who, inputs[f].path, inputs[f].kind, read_err)) break;
            for (bool eof = false; !eof;) {
                Block b;
                if (!free_in.pop(b.buf)) return;
                b.input = f;
                const auto t0 = clk::now();
                const bool ok = rd.next(in_buf[b.buf].p + MASK_HEAD, in_bytes, chunk, b.g, read_err);
                read_s += since(t0);
                if (!ok) { blocks.close(); return; }
                eof = b.g.eof;
                blocks.push(std::move(b));
            }
        }
        blocks.close();
    });
    // writer (only with an output): the last piece is written while the device works on this one
    std::thread writer;
    if (writes) writer = std::thread([&] {
        Piece p;
        while (pieces.pop(p)) {
            const auto t0 = clk::now();
            if (write_err.empty()) write_all(out_fd, p.p, p.len, who, out_name, write_err);
            write_s += since(t0);
            if (p.buf >= 0) free_out.push(p.buf);
        }
    });

    // device: carry + block -> step -> piece
    std::vector<char> carry;
    std::unique_ptr<GzText> gzt;   // gzip: the text and its carry stay on the device
    uint64_t records_before = 0;   // whole records of the current input in front of the current chunk
    size_t cur_input = 0;
    Block b;
    while (err.empty() && blocks.pop(b)) {
        if (b.input != cur_input) { cur_input = b.input; records_before = 0; }
        const ReadsInput &in = inputs[b.input];
        const char *raw = in_buf[b.buf].p + MASK_HEAD;
        Chunk c;
        c.n = carry.size() + b.g.len;
        c.final = b.g.eof;
        c.on_device = in.kind != GZ_KIND_TEXT;
        Piece piece;
        std::shared_ptr<std::vector<char>> big_in;
        if (c.on_device) {
            if (!gzt) gzt.reset(new GzText(ctx));
            const auto t0 = clk::now();
            const bool ok = in.kind == GZ_KIND_GZIP ? gzt->append_plain(who, in.path, raw, b.g.len, b.g.file_off, b.g.eof, err) : gzt->append(who, in.path, raw, b.g, err);
            tm.device_s += since(t0);
            if (!ok) break;
            c.text = gzt->text();
            c.n = gzt->size();
            if (writes && c.n + 1 <= MASK_HEAD + chunk + 16) {
                if (!free_out.pop(piece.buf)) break;
                c.out = out_buf[piece.buf].p;
            } else if (writes) {
                piece.own = std::make_shared<std::vector<char>>(c.n + 1);
                c.out = piece.own->data();
            }
        } else if (carry.size() <= MASK_HEAD) {   // the carried record in front of the block, in place
            char *p = in_buf[b.buf].p + MASK_HEAD - carry.size();
            if (!carry.empty()) memcpy(p, carry.data(), carry.size());
            c.text = p;
            if (writes) {
                if (!free_out.pop(piece.buf)) break;
                c.out = out_buf[piece.buf].p;
            }
        } else {   // a record longer than the room in front: this chunk holds what has gathered so far
            big_in = std::make_shared<std::vector<char>>(c.n);
            memcpy(big_in->data(), carry.data(), carry.size());
            memcpy(big_in->data() + carry.size(), raw, b.g.len);
            c.text = big_in->data();
            if (writes) {
                piece.own = std::make_shared<std::vector<char>>(c.n + 1);
                c.out = piece.own->data();
            }
        }
        c.fasta = in.fasta && starts_fasta(ctx, c.text, c.n, c.on_device);
        Taken t;
        const auto t0 = clk::now();
        const int rc = c.n ? step(c, t) : (int)PF_OK;
        tm.device_s += since(t0);
        if (rc != PF_OK) {
            err = reword_record(pf_last_error(ctx), who, in.path, records_before + t.bad + 1);
            if (piece.buf >= 0) free_out.push(piece.buf);
            break;
        }
        // a chunk that holds no whole record gives used = 0: everything is carried and the next chunk is this one plus the next block
        if (c.on_device) gzt->use(t.used);
        else carry.assign(c.text + t.used, c.text + c.n);
        free_in.push(b.buf);
        records_before += t.reads;
        piece.p = c.out;
        piece.len = t.out_len;
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

// ---- the pair loop's readers ----
struct ReadBlock {
    std::unique_ptr<char[]> p;
    FileBlock g;
};
struct PairReader {   // reads one file block by block, at most two ahead of the device stage
    Chan<int> tokens;
    Chan<ReadBlock> blocks;
    std::string err;
    double read_s = 0;
    std::thread th;
    void start(const std::string &who, const ReadsInput &in, uint64_t chunk) {
        tokens.push(0);
        tokens.push(0);
        th = std::thread([this, who, in, chunk] {
            BlockReader rd;
            if (!rd.open_file(who, in.path, in.kind, err)) { blocks.close(); return; }
            // (a plain-gzip file is read as it is, in smaller blocks: its text is several times its bytes)
            const uint64_t cap = BlockReader::block_bytes(in.kind, chunk);
            for (bool eof = false; !eof;) {
                int token;
                if (!tokens.pop(token)) break;
                ReadBlock b;
                b.p.reset(new char[cap]);
                const auto t0 = clk::now();
                const bool ok = rd.next(b.p.get(), cap, chunk, b.g, err);
                read_s += since(t0);
                if (!ok) break;
                eof = b.g.eof;
                blocks.push(std::move(b));
            }
            blocks.close();
        });
    }
    void stop() {
        tokens.close();
        if (th.joinable()) th.join();
    }
};

}  // namespace

int stream_fastq_pair(pf_ctx *ctx, const char *who_c, const ReadsInput &in1, const ReadsInput &in2, uint64_t chunk_bytes, const PairChunkStep &step,
                      PairStreamTimes &tm, std::string &err) {
    const std::string who = who_c;
    const ReadsInput *in[2] = {&in1, &in2};
    err.clear();
    const bool is_gz[2] = {in1.kind != GZ_KIND_TEXT, in2.kind != GZ_KIND_TEXT};   // (each file of the pair by its own first bytes)
    // a call holds what is pending of each file, up to two blocks of it: both stay below the 2^32 bytes of the device call
    uint64_t chunk = chunk_bytes ? chunk_bytes : MASK_DEFAULT_CHUNK;
    const uint64_t largest = std::max(in1.size, in2.size);
    const uint64_t bound = (is_gz[0] || is_gz[1]) ? std::max<uint64_t>(largest * 8, GZ_MEMBER_MAX) : largest;   // (blocked gzip inflates to a multiple of the file)
    chunk = std::max<uint64_t>(1, std::min<uint64_t>(chunk, std::max<uint64_t>(bound, 1)));
    chunk = std::min<uint64_t>(chunk, 1ull << 30);
    PairReader rd[2];
    rd[0].start(who, in1, chunk);
    rd[1].start(who, in2, chunk);

    std::vector<char> pend[2];             // the carry of each file, then the blocks read behind it
    std::unique_ptr<GzText> gzt[2];        // the same of a gzip file: on the device
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
                if (!rd[f].blocks.pop(b)) { err = !rd[f].err.empty() ? rd[f].err : who + ": reading " + in[f]->path + " ended early"; break; }
                if (is_gz[f]) {
                    const auto t0 = clk::now();
                    const bool ok = in[f]->kind == GZ_KIND_GZIP ? gzt[f]->append_plain(who, in[f]->path, b.p.get(), b.g.len, b.g.file_off, b.g.eof, err)
                                                                : gzt[f]->append(who, in[f]->path, b.p.get(), b.g, err);
                    tm.device_s += since(t0);
                    if (!ok) break;
                } else {
                    pend[f].insert(pend[f].end(), b.p.get(), b.p.get() + b.g.len);
                }
                eof[f] = b.g.eof;
                more[f] = false;
                b.p.reset();
                rd[f].tokens.push(0);
            }
        if (!err.empty()) break;
        PairChunk c;
        c.final = eof[0] && eof[1];
        if (c.final && size_of(0) == 0 && size_of(1) == 0) break;
        // ---- one file has ended and is used up while the other still holds a whole record ----
        for (int f = 0; f < 2 && !c.final; ++f)
            if (eof[f] && size_of(f) == 0 && whole_records(1 - f)) {
                err = who + ": " + in[f]->path + " ends after " + std::to_string(records_before) + " records while " + in[1 - f]->path + " holds more (at least " +
                      std::to_string(records_before + whole_records(1 - f)) + "): the files of a pair hold the same number of records";
            }
        if (!err.empty()) break;
        // ---- the device stage ----
        for (int f = 0; f < 2; ++f) {
            c.text[f] = text_of(f);
            c.n[f] = size_of(f);
            c.on_device[f] = is_gz[f];
        }
        PairTaken t;
        const auto t0 = clk::now();
        const int rc = step(c, t);
        tm.device_s += since(t0);
        if (rc != PF_OK) {
            if (!err.empty()) break;   // (the step has worded it)
            const std::string why = pf_last_error(ctx);
            if (why.find("different numbers of records") != std::string::npos)
                err = who + ": " + in1.path + " holds " + std::to_string(records_before + whole_records(0)) + " records, " + in2.path + " holds " +
                      std::to_string(records_before + whole_records(1)) + ": the files of a pair hold the same number of records";
            else
                err = reword_record(why, who, in[t.bad & 1]->path, records_before + (t.bad >> 1) + 1);
            break;
        }
        for (int f = 0; f < 2; ++f) {
            if (is_gz[f]) gzt[f]->use(t.used[f]);
            else pend[f].erase(pend[f].begin(), pend[f].begin() + (ptrdiff_t)t.used[f]);
        }
        records_before += t.reads;
        if (c.final) break;
        if (t.reads == 0) more[0] = more[1] = true;   // no whole pair: a file that can grows by the next block
    }
    // wind down: on an error the threads are let go first
    for (int f = 0; f < 2; ++f) rd[f].stop();
    for (int f = 0; f < 2 && err.empty(); ++f) err = rd[f].err;
    tm.read_s = std::max(rd[0].read_s, rd[1].read_s);
    return err.empty() ? 0 : 1;
}

}  // namespace pfh
