// What every reads sub-command shares: FASTQ / FASTA files, as text or gzip, streamed through a device call in chunks.
//   fastq_preflight     every input looked at once, before a device context exists: what is refused, and what each input is (ReadsInput)
//   stream_fastq        the inputs one after the other: reader thread, device loop, writer thread, a carry across the chunk edge
//   stream_fastq_pair   the two files of a pair in lock step: two reader threads, a carry per file, one device stage
// The readers are BlockReader, the device side of the compressed inputs is GzText (both pf_gz_host.hpp).  Nothing here knows what a step
// computes: `mask`, `count`, `trim`, `build-multi`, `run` and `run-multi` each bring their own.
#pragma once
#include <stdint.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "pf_gz_host.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

constexpr uint64_t MASK_DEFAULT_CHUNK = 256ull << 20;   // bytes of text a device call, when the command line names none

// a hand-over between two threads; close() wakes everybody, pop() then drains what is left and fails
template <typename T>
struct Chan {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<T> q;
    bool closed = false;
    void push(T v) {
        { std::lock_guard<std::mutex> lk(mu); q.push_back(std::move(v)); }
        cv.notify_all();
    }
    bool pop(T &v) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !q.empty() || closed; });
        if (q.empty()) return false;
        v = std::move(q.front());
        q.pop_front();
        return true;
    }
    void close() {
        { std::lock_guard<std::mutex> lk(mu); closed = true; }
        cv.notify_all();
    }
};

// pinned host memory of a context (pageable when that fails: it works, slower)
struct ChunkBuf {
    pf_ctx *ctx = nullptr;
    char *p = nullptr;
    bool pinned = false;
    bool alloc(pf_ctx *c, size_t bytes);
    ChunkBuf() = default;
    ChunkBuf(const ChunkBuf &) = delete;
    ChunkBuf &operator=(const ChunkBuf &) = delete;
    ~ChunkBuf();
};
bool same_file(const std::string &a, const std::string &b);

// ---- the preflight: what an input is, decided once ----
struct ReadsOptions {
    int gz = 0;           // 0: gzip is refused.  1 (`--gz`): an input with the gzip magic is blocked gzip (pf_inflate::file_clause_gz) or refused by
                          // the clause of its first member.  2 (`--gz-plain`): any other gzip is taken as well (pf_gunzip::file_kind) and refused
                          // only for its method, a reserved flag or a cut header
    bool fasta = false;   // `--fasta`: a first byte of '>' is no refusal
};
struct ReadsInput {
    std::string path;
    uint64_t size = 0;
    GzKind kind = GZ_KIND_TEXT;
    bool fasta = false;   // ReadsOptions::fasta: the stream looks at the first byte of every chunk (Chunk::fasta)
};
// The refusals that need no device, every input looked at before anything is written: no input, an input that cannot be read, FASTA,
// gzip, an input that is one of `outputs`.  `what`: the last word of the FASTA / gzip texts ("masked", "counted").  Every input without
// the gzip magic, and every input without opt.gz, is judged by its first two bytes (pf_mask::file_clause).  0 = ok and `inputs` holds
// one entry per path, in order: the streams below take them (or any run of them) as they are, as often as the sub-command streams.
int fastq_preflight(const char *who, const char *what, const std::vector<std::string> &paths, const std::vector<std::string> &outputs,
                    const ReadsOptions &opt, std::vector<ReadsInput> &inputs, std::string &err);

// ---- one file after the other ----
// One chunk for the device: text[0, n), final = the input ends with it.  on_device: the text is device memory (a gzip input, inflated
// there).  fasta (inputs that allow it alone): the chunk's first byte is '>' -- FASTA (../pf_fasta_rule.hpp); anything else goes the
// FASTQ way.  That holds for every chunk, not only the first: chunks and carries start at record starts.  (On the device the look
// costs a copy of one byte.)  out: where output bytes go, n + 1 of them at most (null without an output).
struct Chunk {
    const char *text = nullptr;
    uint64_t n = 0;
    bool final = false, on_device = false, fasta = false;
    char *out = nullptr;
};
// What a step took: used (bytes of whole records), reads (records), out_len (bytes of `out` the writer gets: used, or fewer where
// records are shortened or dropped); with a status other than PF_OK, bad = the 0-based offender within the chunk.
struct Taken {
    uint64_t used = 0, reads = 0, bad = 0, out_len = 0;
};
// PF_OK or the device call's status (pf_last_error words it)
typedef std::function<int(const Chunk &c, Taken &t)> ChunkStep;
struct StreamTimes {
    double device_s = 0, read_s = 0, write_s = 0;
};
// Reader thread, device loop and (out_fd >= 0) writer thread over two pinned buffers each way, with the carry of a record across a
// chunk edge; out_len bytes of `out` of every chunk go to out_fd in order.  chunk_bytes = 0: MASK_DEFAULT_CHUNK; never more than the
// largest input holds.  0 = ok, else worded in err (format refusals name the input and the 1-based record from the start of that
// input).  A blocked-gzip input: the reader packs whole members, K-INFLATE writes their text on the device behind the carried record,
// and the step gets a device pointer (pf_gz_host.hpp); chunk_bytes then counts inflated bytes, and a refused member is worded
// `who: path: member N, byte B: clause`.  A plain-gzip input is read in raw blocks and inflated by K-GUNZIP (GzText::append_plain).
int stream_fastq(pf_ctx *ctx, const char *who, const std::vector<ReadsInput> &inputs, uint64_t chunk_bytes, int out_fd, const std::string &out_name,
                 const ChunkStep &step, StreamTimes &tm, std::string &err);

// ---- the two files of a pair in lock step ----
// One device call on what is pending of both files, for `trim` and for `run STEP...` / `run-multi STEP...` alike.  The step reports the
// bytes it used of each file, the pairs it took and, with a status other than PF_OK, bad = 2 * record + file of a format refusal.
struct PairChunk {
    const char *text[2] = {nullptr, nullptr};
    uint64_t n[2] = {0, 0};
    bool final = false, on_device[2] = {false, false};
};
struct PairTaken {
    uint64_t used[2] = {0, 0}, reads = 0, bad = 0;
};
typedef std::function<int(const PairChunk &c, PairTaken &t)> PairChunkStep;
struct PairStreamTimes {
    double device_s = 0;   // inside the step
    double read_s = 0;     // read() of the inputs, the slower of the two
};
// Two reader threads, a carry per file, one device stage.  A refusal is worded by `who` with the input's path and the 1-based record
// (files that end at different record counts: with the counts); a step that has worded err itself keeps its words.
int stream_fastq_pair(pf_ctx *ctx, const char *who, const ReadsInput &in1, const ReadsInput &in2, uint64_t chunk_bytes, const PairChunkStep &step,
                      PairStreamTimes &tm, std::string &err);

}  // namespace pfh
