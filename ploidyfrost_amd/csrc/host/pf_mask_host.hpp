// `ploidyfrost mask`: the host side of K-MASK (pf_mask_reads / pf_mask_fastq in ploidyfrost_hip.h, the rule in ../pf_mask_rule.hpp) --
// `kmc_tools filter -hm <db> <reads.fq> -ci<L>` of the reference's workflow (README step 2, script/pipeline/3.filter) against a
// database that is decoded once and looked up in HBM.  (The host's plain restatement of the rule, pf_mask::mask_read and
// pf_mask::index_fastq, lives in the rule header itself.)
#pragma once
#include <stdint.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "ploidyfrost_hip.h"

namespace pfh {

struct CountOptions;   // pf_count_host.hpp

struct MaskTimes {
    double load_s = 0;     // database: map, decode, histogram, table (with -k: the count of the inputs instead)
    double stream_s = 0;   // first byte read to last byte written (wall)
    double device_s = 0;   // of it: inside pf_mask_fastq (upload, kernels, download)
    double read_s = 0;     // of it, beside the device: read() of the inputs
    double write_s = 0;    // of it, beside the device: write() of the output
};

constexpr uint64_t MASK_DEFAULT_CHUNK = 256ull << 20;

// Masks the inputs, one after the other, into out_path (written under a temporary name, renamed at the end; nothing is left under
// either name after a refusal).  auto_lower: low = max(10, cutoffL) of the database's own histogram (K-HIST), as `cutoffL -d` prints
// it.  chunk_bytes = 0: MASK_DEFAULT_CHUNK.  0 = ok, else worded in err (format refusals name the input and the 1-based record).
int mask_fastq(const std::string &db_prefix, const std::vector<std::string> &inputs, const std::string &out_path, uint32_t low, uint32_t up,
               bool auto_lower, uint64_t chunk_bytes, int device, pf_mask_stats &stats, uint32_t &lower_used, MaskTimes *times, std::string &err);
// The same without a database (`mask -k`): the inputs are counted first (K-COUNT, pf_count_host.hpp), the finished counters give the
// histogram and the table, and the inputs are streamed a second time through K-MASK -- what `count ... -o db` followed by
// `mask -d db ...` gives.  db_out (may be empty): the database is written as well.
int mask_fastq_counted(const CountOptions &count, const std::string &db_out, const std::vector<std::string> &inputs, const std::string &out_path,
                       uint32_t low, uint32_t up, bool auto_lower, uint64_t chunk_bytes, int device, pf_mask_stats &stats, uint32_t &lower_used,
                       MaskTimes *times, std::string &err);

// ---- what `mask`, `count` and `trim` share: FASTQ files streamed through a device call in chunks ----
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
// The refusals that need no device, every input looked at before anything is written: no input, an input that cannot be read, FASTA,
// gzip, an input that is one of `outputs`.  `what`: the last word of the FASTA / gzip texts ("masked", "counted").  largest: the size
// of the largest input.  gz (`--gz`): an input with the gzip magic is blocked gzip (pf_inflate::file_clause_gz) or refused by the
// clause of its first member; every other input, and every input without gz, goes the way above, byte for byte.  gz = 2
// (`--gz-plain`): any other gzip is taken as well (pf_gunzip::file_kind) and refused only for its method, a reserved flag or a cut header.
// fasta (`--fasta`): a first byte of '>' is no refusal (an inflated input's kind shows only in the stream: the step decides).
int fastq_preflight(const char *who, const char *what, const std::vector<std::string> &inputs, const std::vector<std::string> &outputs,
                    uint64_t &largest, std::string &err, int gz = 0, bool fasta = false);
// `--fasta`: the kind of a chunk is its first byte -- '>' is FASTA (../pf_fasta_rule.hpp), anything else goes the FASTQ way.  That holds
// for every chunk, not only the first: chunks and carries start at record starts.  on_device (StreamTimes::text_on_device): the text
// is device memory and the look costs a copy of one byte.
bool chunk_is_fasta(pf_ctx *ctx, const char *text, uint64_t n, bool on_device);
// One chunk on the device: text[0, n), final = the input ends with it; out = where output bytes go (null without an output).  Fills
// used (bytes of whole records), reads (records), bad (0-based offender within the chunk); PF_OK or the call's status (pf_last_error).
typedef std::function<int(const char *text, uint64_t n, bool final, char *out, uint64_t &used, uint64_t &reads, uint64_t &bad)> ChunkStep;
struct StreamTimes {
    double device_s = 0, read_s = 0, write_s = 0;
    bool text_on_device = false;   // set before every step: the chunk's text is device memory (a blocked-gzip input, inflated there)
};
// Reader thread, device loop and (out_fd >= 0) writer thread over two pinned buffers each way, with the carry of a record across a
// chunk edge; the used bytes of `out` of every chunk go to out_fd in order.  0 = ok, else worded in err (format refusals name the
// input and the 1-based record from the start of that input).  gz: the inputs that start with the gzip magic are blocked gzip -- the
// reader packs whole members, K-INFLATE writes their text on the device behind the carried record, and the step gets a device
// pointer (pf_gz_host.hpp); chunk_bytes then counts inflated bytes, and a refused member is worded `who: path: member N, byte B: clause`.
// gz = 2: plain-gzip inputs are read in raw blocks and inflated by K-GUNZIP (GzText::append_plain).
int stream_fastq(pf_ctx *ctx, const char *who, const std::vector<std::string> &inputs, uint64_t chunk_bytes, uint64_t largest, int out_fd,
                 const std::string &out_name, const ChunkStep &step, StreamTimes &tm, std::string &err, int gz = 0);

// The same for a step whose output is not as long as its input (`trim`: records are shortened or dropped): out holds n + 1 bytes, and
// the step says in out_len how many of them the writer gets.  stream_fastq is this with out_len = used.
typedef std::function<int(const char *text, uint64_t n, bool final, char *out, uint64_t &used, uint64_t &reads, uint64_t &bad, uint64_t &out_len)> SizedChunkStep;
int stream_fastq_sized(pf_ctx *ctx, const char *who, const std::vector<std::string> &inputs, uint64_t chunk_bytes, uint64_t largest, int out_fd,
                       const std::string &out_name, const SizedChunkStep &step, StreamTimes &tm, std::string &err, int gz = 0);

}  // namespace pfh
